// cross_check.hip -- cross-view consistency check between the maps of several
// reference cameras.
//
// One thread per (view a, pixel p), 256 consecutive pixels per workgroup.  The
// thread reads s = disps[a][p] and walks the other views b in ascending order:
// e = step[b] - step[a] comes from the kernel arguments (uniform over the
// workgroup, so the walk never diverges), q = p + s * e is the pixel of view b
// that sees the same point, and t = disps[b][q] agrees, conflicts or is
// occluded (cross_check_math.h).  Where s is locally constant, neighbouring
// lanes gather neighbouring u16 values of one row.  Nothing is indexed by a
// value held in a vector register; every access is of the element's own size
// (u16 planes at odd W are only 2-byte aligned), so no alignment is assumed.
// Bytes per (view, pixel): 2 read + 2 written (+ 4 + 4 with the f32 plane, + 1
// per count plane) of compulsory traffic, and up to 2 * (n - 1) gathered.
//
// Block order (tune::kCrossTileMajor, measured in §4.21): view-major walks view
// 0's tiles, then view 1's; tile-major puts the view index innermost in groups
// of 8 tiles, so that the workgroups b, b + 8, b + 16 ... -- which the
// dispatcher is observed to place on one XCD -- work on one tile of every view
// in turn and gather from the band of rows that XCD's L2 already holds.  The
// order changes speed only, never a result.
#include "cross_check_math.h"
#include "sva_internal.h"

namespace sva {
namespace {

struct CrossSteps {
    int32_t v[cc::kMaxViews][2];   // view_step, by value like fuse.hip's FuseNum
};

constexpr int kTile = 256;         // pixels (threads) per workgroup
constexpr unsigned kXcdSlots = 8;  // workgroups b and b + 8 share an XCD

__global__ __launch_bounds__(kTile) void cross_check_kernel(
    const uint16_t* __restrict__ disps, const float* __restrict__ subpix, int n, int W, int H,
    unsigned np, unsigned tiles, int tile_major, CrossSteps st, unsigned invalid, int max_diff,
    int min_agree, int max_conflict, uint16_t* __restrict__ out, float* __restrict__ out_sub,
    uint8_t* __restrict__ agree, uint8_t* __restrict__ conflict) {
    unsigned a, tile;
    if (tile_major) {
        const unsigned slot = blockIdx.x % kXcdSlots, rest = blockIdx.x / kXcdSlots;
        a = rest % (unsigned)n;
        tile = (rest / (unsigned)n) * kXcdSlots + slot;
        if (tile >= tiles) return;   // the last group of 8 may be short
    } else {
        a = blockIdx.x / tiles;
        tile = blockIdx.x % tiles;
    }
    const unsigned p = tile * kTile + threadIdx.x;
    if (p >= np) return;
    const size_t ap = (size_t)a * np + p;
    const unsigned s = disps[ap];
    const bool ok = cc::valid(s, invalid);
    const int px = (int)(p % (unsigned)W), py = (int)(p / (unsigned)W);
    const int ax = st.v[a][0], ay = st.v[a][1];
    int na = 0, nc = 0;
#pragma unroll 4
    for (int b = 0; b < n; b++) {
        const int ex = st.v[b][0] - ax, ey = st.v[b][1] - ay;
        int qx = 0, qy = 0;
        const bool in = ok && b != (int)a && cc::inside(px, py, (int)s, ex, ey, W, H, &qx, &qy);
        // (qy, qx) is inside the image here, so the index is below np
        const unsigned t = in ? disps[(size_t)b * np + (size_t)qy * W + qx] : 0u;
        const int cls = in ? cc::classify((int)s, t, invalid, max_diff) : (int)cc::kNone;
        na += cls == cc::kAgree;
        nc += cls == cc::kConflict;
    }
    const bool kept = !ok || cc::keep(na, nc, min_agree, max_conflict);
    out[ap] = (uint16_t)(kept ? s : invalid);
    if (out_sub) out_sub[ap] = kept ? subpix[ap] : __builtin_nanf("");
    if (agree) agree[ap] = (uint8_t)na;
    if (conflict) conflict[ap] = (uint8_t)nc;
}

}  // namespace

hipError_t launch_cross_check(Ctx& c, const uint16_t* disps, const float* subpix, int n, int W,
                              int H, const int32_t* view_step, uint16_t invalid, int max_diff,
                              int min_agree, int max_conflict, int tile_major, uint16_t* out,
                              float* out_sub, uint8_t* agree, uint8_t* conflict) {
    const unsigned long long np64 = (unsigned long long)W * (unsigned long long)H;
    if (n < 1 || n > cc::kMaxViews || W <= 0 || H <= 0 || np64 >= (1ull << 31) || !view_step ||
        max_diff < 0 || (out_sub && !subpix))
        return hipErrorInvalidValue;
    ScopedKernelTimer t(c, "cross_check");
    CrossSteps k{};
    for (int i = 0; i < n; i++) {
        k.v[i][0] = view_step[2 * i];
        k.v[i][1] = view_step[2 * i + 1];
    }
    const unsigned np = (unsigned)np64, tiles = (np + kTile - 1) / kTile;
    // at most 32 * 2^23 workgroups
    const unsigned groups = (tiles + kXcdSlots - 1) / kXcdSlots;
    const unsigned blocks = (tile_major ? groups * kXcdSlots : tiles) * (unsigned)n;
    hipLaunchKernelGGL(cross_check_kernel, dim3(blocks), dim3(kTile), 0, c.stream, disps, subpix, n,
                       W, H, np, tiles, tile_major, k, (unsigned)invalid,
                       max_diff > cc::kMaxDiff ? cc::kMaxDiff : max_diff, min_agree, max_conflict,
                       out, out_sub, agree, conflict);
    return hipGetLastError();
}

}  // namespace sva
