// fuse.hip -- multi-pair depth fusion on the root.
//
// depth(p) = median over maps i with disp_i(p) != invalid and disp_i(p) > 0 of
//            (baseline_i * f) / ((double)disp_i(p) * pixel_size)
// (mean of the two middle values for an even count, 0 if no map is valid).
// One thread per pixel.  The n <= NM depths live in registers (fully unrolled);
// the median is chosen by rank counting (rank_i = #{j : z_j < z_i, or z_j == z_i
// and j < i}), O(NM^2) f64 compares, no data-dependent indexing so nothing
// spills to scratch.  Invalid entries are +inf and rank after every valid one.
// HBM bytes per pixel: 2 * n_maps read + 9 written.  f64 without contraction,
// IEEE division: the same bits as the oracle's insertion sort + mean.
// fuse_depth_conf_kernel (§2.6b) picks one map per pixel by the WTA's
// confidence planes instead: min-cost or max-margin.  fuse_depth_sub_kernel and
// fuse_depth_conf_sub_kernel (§2.6c) are the two with the depth taken from the
// f32 sub-pixel maps.
#include "sva_internal.h"

#pragma clang fp contract(off)

namespace sva {
namespace {

struct FuseNum {
    double v[32];  // baseline_i * f
};

template <int NM>
__global__ __launch_bounds__(256) void fuse_depth_kernel(const uint16_t* __restrict__ disps,
                                                         int n_maps, size_t np, FuseNum num,
                                                         double pixel_size, uint16_t invalid,
                                                         double* __restrict__ depth,
                                                         uint8_t* __restrict__ n_valid) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    double z[NM];
    int n = 0;
#pragma unroll
    for (int i = 0; i < NM; i++) {
        const unsigned d = i < n_maps ? disps[(size_t)i * np + p] : invalid;
        const bool ok = d != invalid && d != 0;
        z[i] = ok ? num.v[i] / ((double)d * pixel_size) : __builtin_inf();
        n += ok;
    }
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
    if (n_valid) n_valid[p] = (uint8_t)n;
}

// Cost-aware fusion: the depth of ONE map per pixel, the
// valid map (§2.6's rule) with the smallest cost_min (MARGIN = false) or the
// largest cost_second - cost_min in u32 (MARGIN = true); ties go to the lowest
// map index (the scan is ascending and only a strictly better map replaces the
// winner).  The winner's disparity, numerator and index move through selects,
// so nothing is indexed by data.  Bytes per pixel: 4 or 6 * n_maps read, 10
// written.  The same f64 expression as the median kernel, no contraction.
template <int NM, bool MARGIN>
__global__ __launch_bounds__(256) void fuse_depth_conf_kernel(
    const uint16_t* __restrict__ disps, const uint16_t* __restrict__ cost_min,
    const uint16_t* __restrict__ cost_second, int n_maps, size_t np, FuseNum num,
    double pixel_size, uint16_t invalid, double* __restrict__ depth,
    uint8_t* __restrict__ n_valid, uint8_t* __restrict__ winner) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    int n = 0, wi = 0xff;
    unsigned wd = 0u, wscore = 0u;
    double wnum = 0.0;
#pragma unroll
    for (int i = 0; i < NM; i++) {
        const bool in = i < n_maps;
        const unsigned d = in ? disps[(size_t)i * np + p] : invalid;
        const bool ok = d != invalid && d != 0;
        unsigned score = in ? cost_min[(size_t)i * np + p] : 0u;
        if constexpr (MARGIN) score = (in ? (unsigned)cost_second[(size_t)i * np + p] : 0u) - score;
        const bool take = ok && (n == 0 || (MARGIN ? score > wscore : score < wscore));
        wd = take ? d : wd;
        wscore = take ? score : wscore;
        wnum = take ? num.v[i] : wnum;
        wi = take ? i : wi;
        n += ok;
    }
    depth[p] = n == 0 ? 0.0 : wnum / ((double)wd * pixel_size);
    if (n_valid) n_valid[p] = (uint8_t)n;
    if (winner) winner[p] = (uint8_t)wi;
}

// Sub-pixel fusion: the two kernels above with the depth taken
// from the f32 sub-pixel disparity s_i of §2.4 in place of the u16 one.  Map i
// is valid where d_i != invalid, d_i != 0 and s_i > 0.0f -- false for the NaN of
// a rejected pixel, so no NaN reaches the rank count -- and its depth is
// num_i / ((double)s_i * pixel_size).  (double)(float)d == (double)d for a u16,
// so planes with s_i == (float)d_i give the bits of the kernels above.  Bytes per
// pixel: 6 * n_maps read + 9 written; the cost-aware form 8 or 10 * n_maps + 10.
template <int NM>
__global__ __launch_bounds__(256) void fuse_depth_sub_kernel(
    const uint16_t* __restrict__ disps, const float* __restrict__ subpix, int n_maps, size_t np,
    FuseNum num, double pixel_size, uint16_t invalid, double* __restrict__ depth,
    uint8_t* __restrict__ n_valid) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    double z[NM];
    int n = 0;
#pragma unroll
    for (int i = 0; i < NM; i++) {
        const bool in = i < n_maps;
        const unsigned d = in ? disps[(size_t)i * np + p] : invalid;
        const float s = in ? subpix[(size_t)i * np + p] : 0.0f;
        const bool ok = d != invalid && d != 0 && s > 0.0f;
        z[i] = ok ? num.v[i] / ((double)s * pixel_size) : __builtin_inf();
        n += ok;
    }
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
    if (n_valid) n_valid[p] = (uint8_t)n;
}

// The winner is chosen as in fuse_depth_conf_kernel (the cost planes decide,
// ties to the lowest index) among the maps valid by the rule above; its
// sub-pixel disparity moves through the selects in place of the u16 one.
template <int NM, bool MARGIN>
__global__ __launch_bounds__(256) void fuse_depth_conf_sub_kernel(
    const uint16_t* __restrict__ disps, const float* __restrict__ subpix,
    const uint16_t* __restrict__ cost_min, const uint16_t* __restrict__ cost_second, int n_maps,
    size_t np, FuseNum num, double pixel_size, uint16_t invalid, double* __restrict__ depth,
    uint8_t* __restrict__ n_valid, uint8_t* __restrict__ winner) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    int n = 0, wi = 0xff;
    unsigned wscore = 0u;
    float ws = 0.0f;
    double wnum = 0.0;
#pragma unroll
    for (int i = 0; i < NM; i++) {
        const bool in = i < n_maps;
        const unsigned d = in ? disps[(size_t)i * np + p] : invalid;
        const float s = in ? subpix[(size_t)i * np + p] : 0.0f;
        const bool ok = d != invalid && d != 0 && s > 0.0f;
        unsigned score = in ? cost_min[(size_t)i * np + p] : 0u;
        if constexpr (MARGIN) score = (in ? (unsigned)cost_second[(size_t)i * np + p] : 0u) - score;
        const bool take = ok && (n == 0 || (MARGIN ? score > wscore : score < wscore));
        ws = take ? s : ws;
        wscore = take ? score : wscore;
        wnum = take ? num.v[i] : wnum;
        wi = take ? i : wi;
        n += ok;
    }
    depth[p] = n == 0 ? 0.0 : wnum / ((double)ws * pixel_size);
    if (n_valid) n_valid[p] = (uint8_t)n;
    if (winner) winner[p] = (uint8_t)wi;
}

}  // namespace

hipError_t launch_fuse_depth_conf(Ctx& c, const uint16_t* disps, const uint16_t* cost_min,
                                  const uint16_t* cost_second, int n_maps, size_t np,
                                  const double* num, double pixel_size, uint16_t invalid, int mode,
                                  double* depth, uint8_t* n_valid, uint8_t* winner) {
    if (n_maps < 1 || n_maps > 32) return hipErrorInvalidValue;
    if (mode != SVA_FUSE_MIN_COST && mode != SVA_FUSE_MAX_MARGIN) return hipErrorInvalidValue;
    if (mode == SVA_FUSE_MAX_MARGIN && !cost_second) return hipErrorInvalidValue;
    ScopedKernelTimer t(c, "fuse_depth_conf");
    FuseNum k{};
    for (int i = 0; i < n_maps; i++) k.v[i] = num[i];
    const dim3 grid((unsigned)((np + 255) / 256));
#define SVA_FUSE_C(NM, MG)                                                                       \
    hipLaunchKernelGGL((fuse_depth_conf_kernel<NM, MG>), grid, dim3(256), 0, c.stream, disps,    \
                       cost_min, cost_second, n_maps, np, k, pixel_size, invalid, depth, n_valid, \
                       winner)
#define SVA_FUSE_N(MG)                    \
    do {                                  \
        if (n_maps <= 4) SVA_FUSE_C(4, MG);        \
        else if (n_maps <= 8) SVA_FUSE_C(8, MG);   \
        else if (n_maps <= 16) SVA_FUSE_C(16, MG); \
        else SVA_FUSE_C(32, MG);                   \
    } while (0)
    if (mode == SVA_FUSE_MAX_MARGIN) SVA_FUSE_N(true);
    else SVA_FUSE_N(false);
#undef SVA_FUSE_N
#undef SVA_FUSE_C
    return hipGetLastError();
}

hipError_t launch_fuse_depth(Ctx& c, const uint16_t* disps, int n_maps, size_t np,
                             const double* num, double pixel_size, uint16_t invalid,
                             double* depth, uint8_t* n_valid) {
    if (n_maps < 1 || n_maps > 32) return hipErrorInvalidValue;
    ScopedKernelTimer t(c, "fuse_depth");
    FuseNum k{};
    for (int i = 0; i < n_maps; i++) k.v[i] = num[i];
    const dim3 grid((unsigned)((np + 255) / 256));
#define SVA_FUSE(NM) \
    hipLaunchKernelGGL(fuse_depth_kernel<NM>, grid, dim3(256), 0, c.stream, disps, n_maps, np, k, \
                       pixel_size, invalid, depth, n_valid)
    if (n_maps <= 4) SVA_FUSE(4);
    else if (n_maps <= 8) SVA_FUSE(8);
    else if (n_maps <= 16) SVA_FUSE(16);
    else SVA_FUSE(32);
#undef SVA_FUSE
    return hipGetLastError();
}

hipError_t launch_fuse_depth_conf_sub(Ctx& c, const uint16_t* disps, const float* subpix,
                                      const uint16_t* cost_min, const uint16_t* cost_second,
                                      int n_maps, size_t np, const double* num, double pixel_size,
                                      uint16_t invalid, int mode, double* depth, uint8_t* n_valid,
                                      uint8_t* winner) {
    if (n_maps < 1 || n_maps > 32 || !subpix) return hipErrorInvalidValue;
    if (mode != SVA_FUSE_MIN_COST && mode != SVA_FUSE_MAX_MARGIN) return hipErrorInvalidValue;
    if (mode == SVA_FUSE_MAX_MARGIN && !cost_second) return hipErrorInvalidValue;
    ScopedKernelTimer t(c, "fuse_depth_conf_sub");
    FuseNum k{};
    for (int i = 0; i < n_maps; i++) k.v[i] = num[i];
    const dim3 grid((unsigned)((np + 255) / 256));
#define SVA_FUSE_C(NM, MG)                                                                        \
    hipLaunchKernelGGL((fuse_depth_conf_sub_kernel<NM, MG>), grid, dim3(256), 0, c.stream, disps, \
                       subpix, cost_min, cost_second, n_maps, np, k, pixel_size, invalid, depth,  \
                       n_valid, winner)
#define SVA_FUSE_N(MG)                             \
    do {                                           \
        if (n_maps <= 4) SVA_FUSE_C(4, MG);        \
        else if (n_maps <= 8) SVA_FUSE_C(8, MG);   \
        else if (n_maps <= 16) SVA_FUSE_C(16, MG); \
        else SVA_FUSE_C(32, MG);                   \
    } while (0)
    if (mode == SVA_FUSE_MAX_MARGIN) SVA_FUSE_N(true);
    else SVA_FUSE_N(false);
#undef SVA_FUSE_N
#undef SVA_FUSE_C
    return hipGetLastError();
}

hipError_t launch_fuse_depth_sub(Ctx& c, const uint16_t* disps, const float* subpix, int n_maps,
                                 size_t np, const double* num, double pixel_size, uint16_t invalid,
                                 double* depth, uint8_t* n_valid) {
    if (n_maps < 1 || n_maps > 32 || !subpix) return hipErrorInvalidValue;
    ScopedKernelTimer t(c, "fuse_depth_sub");
    FuseNum k{};
    for (int i = 0; i < n_maps; i++) k.v[i] = num[i];
    const dim3 grid((unsigned)((np + 255) / 256));
#define SVA_FUSE(NM)                                                                             \
    hipLaunchKernelGGL(fuse_depth_sub_kernel<NM>, grid, dim3(256), 0, c.stream, disps, subpix,   \
                       n_maps, np, k, pixel_size, invalid, depth, n_valid)
    if (n_maps <= 4) SVA_FUSE(4);
    else if (n_maps <= 8) SVA_FUSE(8);
    else if (n_maps <= 16) SVA_FUSE(16);
    else SVA_FUSE(32);
#undef SVA_FUSE
    return hipGetLastError();
}

}  // namespace sva
