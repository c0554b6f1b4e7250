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
#include "cost_fuse_math.h"
#include "sva_device.h"
#include "sva_internal.h"

namespace sva {
namespace {

typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef const v4u __attribute__((address_space(1))) gv4u;   // global memory

struct FuseSteps {
    short sx[32], sy[32];
};

// NC = D / 16 lanes per pixel; NM = pair-count class (n <= NM).
template <int NC, int NM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void cost_fuse_kernel(
    const uint8_t* __restrict__ volumes, size_t stride, int n, int W, int H, unsigned nlanes,
    int dmin, int dreal, FuseSteps steps, uint8_t* __restrict__ fused) {
    constexpr int D = NC * 16;
    __shared__ unsigned magic[33];
    if (threadIdx.x < 33) magic[threadIdx.x] = mb::mean_magic((int)threadIdx.x);
    __syncthreads();
    const unsigned lane = blockIdx.x * 256u + threadIdx.x;
    if (lane >= nlanes) return;
    const unsigned pix = lane / NC;
    const int c = (int)(lane - pix * NC);
    const int y = (int)(pix / (unsigned)W), x = (int)(pix - (unsigned)y * (unsigned)W);
    const int d0 = 16 * c;
    const unsigned off = lane * 16u;   // < W*H*D < 2^32: inside one volume

    unsigned E[4] = {0, 0, 0, 0}, O[4] = {0, 0, 0, 0}, cnt[4] = {0, 0, 0, 0};
    auto load4 = [&](int i0, v4u (&v)[4]) {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (i0 + j < n) {   // uniform
                // 64-bit and uniform; pinned to a scalar pair so that the load
                // is "scalar base + 32-bit lane offset", not a 64-bit add per lane
                uint64_t base = (uint64_t)volumes + (uint64_t)(i0 + j) * stride;
                asm("" : "+s"(base));
                v[j] = __builtin_nontemporal_load((gv4u*)(base + off));
            }
    };
    auto sum4 = [&](int i0, const v4u (&v)[4]) {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (i0 + j < n) {   // uniform
                const int lim = mb::pair_lim(x, y, W, H, steps.sx[i0 + j], steps.sy[i0 + j], dmin, D);
                const int k = lim - d0;   // visible bytes of this lane: the first k
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int kq = k - 4 * q;
                    const unsigned mask =
                        kq >= 4 ? 0xffffffffu : (kq <= 0 ? 0u : (1u << (8 * kq)) - 1u);
                    const unsigned w = v[j][q] & mask;
                    E[q] += w & 0x00ff00ffu;
                    O[q] += (w >> 8) & 0x00ff00ffu;
                    cnt[q] += mask & 0x04040404u;
                }
            }
    };
    v4u cur[4] = {}, nxt[4] = {};
    load4(0, cur);
#pragma unroll
    for (int i0 = 0; i0 < NM; i0 += 4) {
        if (i0 + 4 < NM && i0 + 4 < n) load4(i0 + 4, nxt);
        if (i0 < n) sum4(i0, cur);
#pragma unroll
        for (int j = 0; j < 4; j++) cur[j] = nxt[j];
    }

    unsigned out[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        unsigned w = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const unsigned n4 = (cnt[q] >> (8 * b)) & 0xffu;   // 4 * n = the magic's LDS offset
            const unsigned s = ((b & 1 ? O[q] : E[q]) >> (16 * (b >> 1))) & 0xffffu;
            const unsigned mg = *(const unsigned*)((const char*)magic + n4);
            const unsigned r = n4 ? mb::mean_round(2u * s + (n4 >> 2), mg) : 62u;
            w |= r << (8 * b);
        }
        out[q] = w | pad_bytes(d0 + 4 * q, dreal);
    }
    *(v4u*)(fused + off) = (v4u){out[0], out[1], out[2], out[3]};
}

}  // namespace

hipError_t launch_cost_fuse(Ctx& c, const uint8_t* volumes, size_t stride, int n, int W, int H,
                            int D, int dreal, int dmin, const int32_t* steps, uint8_t* fused) {
    if (n < 1 || n > 32 || !paths_supported(D)) return hipErrorInvalidValue;
    if (dreal <= 0) dreal = D;
    ScopedKernelTimer t(c, "cost_fuse");
    FuseSteps k{};
    for (int i = 0; i < n; i++) {
        k.sx[i] = (short)steps[2 * i];
        k.sy[i] = (short)steps[2 * i + 1];
    }
    const int nc = D / 16;
    const unsigned nlanes = (unsigned)((size_t)W * H * nc);   // W*H*D < 2^32 (check_sgm)
    const dim3 grid((nlanes + 255u) / 256u);
#define SVA_CF(NC, NM)                                                                          \
    hipLaunchKernelGGL((cost_fuse_kernel<NC, NM>), grid, dim3(256), 0, c.stream, volumes, stride, \
                       n, W, H, nlanes, dmin, dreal, k, fused)
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
        case 16: SVA_CF_N(16); break;
        default: return hipErrorInvalidValue;
    }
#undef SVA_CF_N
#undef SVA_CF
    return hipGetLastError();
}

}  // namespace sva
