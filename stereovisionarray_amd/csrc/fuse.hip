// fuse.hip -- multi-pair depth fusion on the root (DESIGN.md §2.6, §2.6b, §2.6c;
// SURVEY.md §8e).  One kernel, fuse_kernel<NM, MODE, SUB>, one thread per pixel,
// 24 instances: NM = 4, 8, 16, 32 unrolled maps x three modes x two value types.
//
// Map i is valid where disp_i(p) != invalid and disp_i(p) > 0 and, with SUB, the
// f32 sub-pixel disparity s_i(p) of §2.4 is > 0.0f -- false for the NaN of a
// rejected pixel, so no NaN reaches the rank count.  Its depth is
//     z_i = (baseline_i * f) / ((double)v_i * pixel_size),  v_i = SUB ? s_i : disp_i
// in f64 without contraction and with IEEE division: the oracle's bits.
// (double)(float)d == (double)d for a u16, so planes with s_i == (float)disp_i
// give the bits of the u16 form.
//
// SVA_FUSE_MEDIAN (§2.6): the median of the valid z_i (mean of the two middle
// values for an even count, 0 if no map is valid).  The n <= NM depths live in
// registers (fully unrolled); the median is chosen by rank counting (rank_i =
// #{j : z_j < z_i, or z_j == z_i and j < i}), O(NM^2) f64 compares, no
// data-dependent indexing so nothing spills to scratch.  Invalid entries are
// +inf and rank after every valid one: the same bits as the oracle's insertion
// sort + mean.
// SVA_FUSE_MIN_COST, SVA_FUSE_MAX_MARGIN (§2.6b): the depth of ONE map per pixel,
// the valid map with the smallest cost_min or the largest cost_second - cost_min
// in u32; ties go to the lowest map index (the scan is ascending and only a
// strictly better map replaces the winner).  The winner's value, numerator and
// index move through selects, so nothing is indexed by data.
//
// HBM bytes per pixel (u16 form / SUB), n = n_maps: median 2 n + 9 / 6 n + 9;
// min-cost 4 n + 10 / 8 n + 10; max-margin 6 n + 10 / 10 n + 10.
#include "sva_internal.h"

#pragma clang fp contract(off)

namespace sva {
namespace {

struct FuseNum {
    double v[32];  // baseline_i * f
};

// subpix comes last: with it between disps and cost_min the 32-map u16 min-cost
// instance waited on four more of its loads and ran 8 % slower
// (profiles/fuse_fold/).
template <int NM, int MODE, bool SUB>
__global__ __launch_bounds__(256) void fuse_kernel(
    const uint16_t* __restrict__ disps, const uint16_t* __restrict__ cost_min,
    const uint16_t* __restrict__ cost_second, int n_maps, size_t np, FuseNum num,
    double pixel_size, uint16_t invalid, double* __restrict__ depth,
    uint8_t* __restrict__ n_valid, uint8_t* __restrict__ winner,
    const float* __restrict__ subpix) {
    using V = std::conditional_t<SUB, float, unsigned>;   // what feeds (double)v * pixel_size
    constexpr bool MEDIAN = MODE == SVA_FUSE_MEDIAN, MARGIN = MODE == SVA_FUSE_MAX_MARGIN;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    double z[MEDIAN ? NM : 1];
    int n = 0, wi = 0xff;
    unsigned wscore = 0u;
    V wv = 0;
    double wnum = 0.0;
#pragma unroll
    for (int i = 0; i < NM; i++) {
        const bool in = i < n_maps;
        const unsigned d = in ? disps[(size_t)i * np + p] : invalid;
        bool ok = d != invalid && d != 0;
        V v;
        if constexpr (SUB) {
            v = in ? subpix[(size_t)i * np + p] : 0.0f;
            ok = ok && v > 0.0f;
        } else {
            v = d;
        }
        if constexpr (MEDIAN) {
            z[i] = ok ? num.v[i] / ((double)v * pixel_size) : __builtin_inf();
        } else {
            unsigned score = in ? cost_min[(size_t)i * np + p] : 0u;
            if constexpr (MARGIN) score = (in ? (unsigned)cost_second[(size_t)i * np + p] : 0u) - score;
            const bool take = ok && (n == 0 || (MARGIN ? score > wscore : score < wscore));
            wv = take ? v : wv;
            wscore = take ? score : wscore;
            wnum = take ? num.v[i] : wnum;
            wi = take ? i : wi;
        }
        n += ok;
    }
    if constexpr (MEDIAN) {
        const int lo = (n - 1) >> 1, hi = n >> 1;
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int i = 0; i < NM; i++) {
            int r = 0;
#pragma unroll
            for (int j = 0; j < NM; j++)
                if (j != i) r += (z[j] < z[i]) || (j < i && z[j] == z[i]);
            if (r == lo) a = z[i];
            if (r == hi) b = z[i];
        }
        depth[p] = n == 0 ? 0.0 : ((n & 1) ? a : (a + b) * 0.5);
    } else {
        depth[p] = n == 0 ? 0.0 : wnum / ((double)wv * pixel_size);
    }
    if (n_valid) n_valid[p] = (uint8_t)n;
    if constexpr (!MEDIAN)
        if (winner) winner[p] = (uint8_t)wi;
}

}  // namespace

hipError_t launch_fuse(Ctx& c, const uint16_t* disps, const float* subpix, const uint16_t* cost_min,
                       const uint16_t* cost_second, int n_maps, size_t np, const double* num,
                       double pixel_size, uint16_t invalid, int mode, double* depth,
                       uint8_t* n_valid, uint8_t* winner) {
    const bool median = mode == SVA_FUSE_MEDIAN, sub = subpix != nullptr;
    if (n_maps < 1 || n_maps > 32) return hipErrorInvalidValue;
    if (!median && mode != SVA_FUSE_MIN_COST && mode != SVA_FUSE_MAX_MARGIN)
        return hipErrorInvalidValue;
    if (!median && !cost_min) return hipErrorInvalidValue;
    if (mode == SVA_FUSE_MAX_MARGIN && !cost_second) return hipErrorInvalidValue;
    ScopedKernelTimer t(c, median ? (sub ? "fuse_depth_sub" : "fuse_depth")
                                  : (sub ? "fuse_depth_conf_sub" : "fuse_depth_conf"));
    FuseNum k{};
    for (int i = 0; i < n_maps; i++) k.v[i] = num[i];
    const dim3 grid((unsigned)((np + 255) / 256));
    // NM = 1 << L, the smallest of 4, 8, 16, 32 that holds n_maps
    const int log2_nm = n_maps <= 4 ? 2 : n_maps <= 8 ? 3 : n_maps <= 16 ? 4 : 5;
    static_assert(SVA_FUSE_MIN_COST == 0 && SVA_FUSE_MAX_MARGIN == 1 && SVA_FUSE_MEDIAN == 2,
                  "the mode ladder below walks 0..2");
    for_int_in<2, 5>(log2_nm, [&](auto L) {
        for_int_in<0, 2>(mode, [&](auto M) {
            with_flag<true>(sub, [&](auto S) {
                hipLaunchKernelGGL(
                    (fuse_kernel<(1 << decltype(L)::value), decltype(M)::value, decltype(S)::value>),
                    grid, dim3(256), 0, c.stream, disps, cost_min, cost_second, n_maps, np, k,
                    pixel_size, invalid, depth, n_valid, winner, subpix);
            });
        });
    });
    return hipGetLastError();
}

}  // namespace sva
