// cost_fuse.hip -- multi-baseline cost fusion.
//
// N u8 cost volumes [H][W][D] of one reference image, one per matched image,
// become one: per cell the mean, rounded half up, over the pairs whose matched
// pixel lies inside the image at that disparity, 62 where none does, 255 at
// the padded disparities d >= dreal (§4.7).
//
// One lane owns 16 consecutive disparities of one pixel: one dwordx4 load per
// volume, one dwordx4 store.  Volume i starts at volumes + i * stride, formed
// in 64 bits from uniform values (a scalar base per volume); the lane's own
// offset, 16 * lane, stays below 2^32 inside one volume.  The loads of four
// volumes are in flight before the first is used, and the next four are issued
// before the current four are summed.  The pair volumes are read once and
// never again (non-temporal loads); the fused volume is the next kernel's
// input (plain store).
//
// A pair is visible at d < lim_i(p) (cost_fuse_math.h), so within a lane its
// visible bytes are a prefix of the 16: a byte mask per dword.  Sums are SWAR:
// the even and the odd bytes of a dword accumulate in two packed-u16 pairs
// (32 * 255 fits a u16), the visible-pair counts in packed bytes (4 * n <= 128,
// kept times four: the byte is the LDS address of its divisor's magic).  The
// mean is one 24-bit multiply and a shift per byte, exact for every n and sum
// (mean_round).
//
// HBM bytes per disparity: N read + 1 written.  VALU per lane: about 45 per
// pair (masks, SWAR adds, lim) and about 130 for the 16 divisions; against
// 16 * (N + 1) bytes that stays memory-bound from N = 2 up.
//
// Mixed-baseline groups (§2.2d) run cost_fuse_mixed_kernel: the same text
// (cost_fuse_kernel.inc) with the visibility limit of a pair at a rational
// baseline ratio (mixed_lim).
#include "cost_mixed_math.h"
#include "sva_device.h"
#include "sva_internal.h"

namespace sva {
namespace {

typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef const v4u __attribute__((address_space(1))) gv4u;   // global memory

struct FuseSteps {
    short sx[32], sy[32];
};

// The pairs' baseline ratios of the mixed instance, reduced.
struct FuseRatios {
    unsigned char num[32], den[32];
};

// cost_fuse_kernel<NC, NM>: equal baselines, a pair is visible at d < pair_lim.
#define SVA_FUSE_KERNEL cost_fuse_kernel
#define SVA_FUSE_RATIOS
#define SVA_FUSE_LIM(i) mb::pair_lim(x, y, W, H, steps.sx[i], steps.sy[i], dmin, D)
#include "cost_fuse_kernel.inc"
#undef SVA_FUSE_KERNEL
#undef SVA_FUSE_RATIOS
#undef SVA_FUSE_LIM

// cost_fuse_mixed_kernel<NC, NM>: pair i at ratios.num[i] / ratios.den[i] of
// the unit baseline, visible at d < mixed_lim (§2.2d).
#define SVA_FUSE_KERNEL cost_fuse_mixed_kernel
#define SVA_FUSE_RATIOS FuseRatios ratios,
#define SVA_FUSE_LIM(i) \
    mb::mixed_lim(x, y, W, H, steps.sx[i], steps.sy[i], ratios.num[i], ratios.den[i], dmin, D)
#include "cost_fuse_kernel.inc"
#undef SVA_FUSE_KERNEL
#undef SVA_FUSE_RATIOS
#undef SVA_FUSE_LIM

}  // namespace

// ratios null: cost_fuse_kernel.  Else the mixed instance (§2.2d): ratios[i] =
// (num, den) of pair i, each in 1..8.
hipError_t launch_cost_fuse(Ctx& c, const uint8_t* volumes, size_t stride, int n, int W, int H,
                            int D, int dreal, int dmin, const int32_t* steps,
                            const int32_t* ratios, uint8_t* fused) {
    if (n < 1 || n > 32 || !paths_supported(D)) return hipErrorInvalidValue;
    if (dreal <= 0) dreal = D;
    FuseSteps k{};
    FuseRatios r{};
    for (int i = 0; i < n; i++) {
        k.sx[i] = (short)steps[2 * i];
        k.sy[i] = (short)steps[2 * i + 1];
        if (!ratios) continue;
        const int num = ratios[2 * i], den = ratios[2 * i + 1];
        if (num < 1 || num > mb::kMaxRatio || den < 1 || den > mb::kMaxRatio)
            return hipErrorInvalidValue;
        r.num[i] = (unsigned char)num;
        r.den[i] = (unsigned char)den;
    }
    const int nc = D / 16;
    if (nc != 4 && nc != 8 && nc != 12 && nc != 16) return hipErrorInvalidValue;
    ScopedKernelTimer t(c, "cost_fuse");
    const unsigned nlanes = (unsigned)((size_t)W * H * nc);   // W*H*D < 2^32 (check_sgm)
    const dim3 grid((nlanes + 255u) / 256u);
#define SVA_CF(NC, NM)                                                                          \
    do {                                                                                        \
        if (ratios)                                                                             \
            hipLaunchKernelGGL((cost_fuse_mixed_kernel<NC, NM>), grid, dim3(256), 0, c.stream,  \
                               volumes, stride, n, W, H, nlanes, dmin, dreal, k, r, fused);     \
        else                                                                                    \
            hipLaunchKernelGGL((cost_fuse_kernel<NC, NM>), grid, dim3(256), 0, c.stream,        \
                               volumes, stride, n, W, H, nlanes, dmin, dreal, k, fused);        \
    } while (0)
#define SVA_CF_N(NC)                      \
    do {                                  \
        if (n <= 4) SVA_CF(NC, 4);        \
        else if (n <= 8) SVA_CF(NC, 8);   \
        else if (n <= 16) SVA_CF(NC, 16); \
        else SVA_CF(NC, 32);              \
    } while (0)
    switch (nc) {
        case 4: SVA_CF_N(4); break;
        case 8: SVA_CF_N(8); break;
        case 12: SVA_CF_N(12); break;
        default: SVA_CF_N(16); break;
    }
#undef SVA_CF_N
#undef SVA_CF
    return hipGetLastError();
}

}  // namespace sva
