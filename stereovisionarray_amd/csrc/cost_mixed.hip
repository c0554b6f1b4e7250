// cost_mixed.hip -- Hamming cost volume of a pair whose baseline is a rational
// multiple num/den of its group's unit baseline.
//
// C[(y*W + x)*D + d] = popcount(CL(x,y) ^ CR((x,y) + off(t(dmin + d)))), 62
// where that pixel leaves the image, 255 at d >= dreal (§4.7), from two census
// maps; t(s) = s*num/den rounded half up (cost_mixed_math.h), off the §2.2
// offset of the pair's step.
//
// The matched offset depends on d alone, and consecutive d are no longer
// consecutive words of the matched row (t strides by num/den), so the lattice
// reuse of cost.hip does not apply.  Instead a workgroup owns PX = 64
// consecutive pixels of one row and builds o[d] = off(t(dmin + d)) once in LDS.
// A wave takes a quarter of the disparities; for one d its 64 lanes read the 64
// consecutive census words of row y + o[d].y from column x0 + o[d].x on: one
// 512-byte segment per load instruction, served by L2 / the Infinity Cache (a
// census map is 8 bytes per pixel).  16 such loads are in flight per lane.
// Each lane packs the costs of 4 consecutive d into a dword and writes it to
// an LDS tile [PX][D + 4] bytes: the row pitch of D/4 + 1 dwords is odd, so the
// 32 lanes of a ds_write_b32 group fall on 32 distinct banks (a pitch of D
// bytes would put them on 2 banks at D = 64 and on one from D = 128 up;
// measured at D = 128 that costs only 1-3 %, and 8 loads in flight instead of
// 16 are equal, 32 are 10 % slower: DESIGN.md §4.20).  After one
// barrier the tile -- 64*D contiguous bytes of the volume -- leaves as
// coalesced dwordx4 stores, non-temporal like cost.hip's.
//
// Bytes per cost byte: 8 read from cache (the matched word), 1 written to HBM,
// 2 through LDS.
#include "cost_mixed_math.h"
#include "sva_device.h"
#include "sva_internal.h"

namespace sva {
namespace {

constexpr int kPX = 64;                    // pixels per workgroup: one per lane
constexpr int kInFlight = 16;              // matched words loaded per lane before use
constexpr uint64_t kOutside = 1ull << 63;  // never set in a census word (bits 0..61)

typedef unsigned v4u __attribute__((ext_vector_type(4)));

template <int NC>
__global__ __launch_bounds__(256) void cost_mixed_kernel(
    const uint64_t* __restrict__ cl, const uint64_t* __restrict__ cr, int W, int H, int dmin,
    int sx, int sy, int num, int den, int dreal, int tiles, uint8_t* __restrict__ C) {
    constexpr int D = NC * 16, PITCH = D / 4 + 1, DW = D / 4;   // PITCH in dwords
    __shared__ int2 off[D];
    __shared__ unsigned tile[kPX * PITCH];
    const int t = threadIdx.x;
    const int y = blockIdx.x / tiles, x0 = (blockIdx.x - y * tiles) * kPX;
    for (int d = t; d < D; d += 256)
        off[d] = step_offset(mb::mixed_distance(dmin + d, num, den), sx, sy);
    __syncthreads();
    const int lane = t & 63, wave = t >> 6;
    const int x = x0 + lane;
    if (x < W) {
        const uint64_t l = cl[(size_t)y * W + x];
        unsigned* row = tile + lane * PITCH;
        for (int d0 = wave * DW; d0 < (wave + 1) * DW; d0 += kInFlight) {
            uint64_t w[kInFlight];
#pragma unroll
            for (int k = 0; k < kInFlight; k++) {
                const int2 o = off[d0 + k];   // one address per wave: an LDS broadcast
                const int xr = x + o.x, yr = y + o.y;
                w[k] = ((unsigned)xr < (unsigned)W && (unsigned)yr < (unsigned)H)
                           ? cr[(size_t)yr * W + xr]
                           : kOutside;
            }
#pragma unroll
            for (int q = 0; q < kInFlight / 4; q++) {
                unsigned ww = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const uint64_t v = l ^ w[4 * q + b];
                    const unsigned cst = (v >> 63) ? 62u : (unsigned)__popcll(v);
                    ww |= cst << (8 * b);
                }
                row[(d0 >> 2) + q] = ww | pad_bytes(d0 + 4 * q, dreal);
            }
        }
    }
    __syncthreads();
    // the tile's 64 * D bytes are contiguous in the volume: 16 bytes per lane
    uint8_t* out = C + ((size_t)y * W + x0) * D;
#pragma unroll
    for (int i = t; i < kPX * D / 16; i += 256) {
        const int byte = 16 * i, px = byte / D, dw = (byte - px * D) >> 2;
        if (x0 + px < W) {
            const unsigned* src = tile + px * PITCH + dw;
            __builtin_nontemporal_store((v4u){src[0], src[1], src[2], src[3]}, (v4u*)(out + byte));
        }
    }
}

}  // namespace

hipError_t launch_cost_mixed(Ctx& c, const uint64_t* cen_ref, const uint64_t* cen_oth, int W, int H,
                             int D, int dmin, int sx, int sy, int num, int den, uint8_t* C,
                             int dreal) {
    if (num < 1 || num > mb::kMaxRatio || den < 1 || den > mb::kMaxRatio || W <= 0 || H <= 0 ||
        (sx == 0 && sy == 0))
        return hipErrorInvalidValue;
    if (dreal <= 0) dreal = D;
    ScopedKernelTimer t(c, "cost_mixed");
    const int tiles = (W + kPX - 1) / kPX;
    const dim3 grid((unsigned)tiles * (unsigned)H);   // H <= 65535 (check_sgm)
#define SVA_CM(NC)                                                                            \
    hipLaunchKernelGGL(cost_mixed_kernel<NC>, grid, dim3(256), 0, c.stream, cen_ref, cen_oth, W, \
                       H, dmin, sx, sy, num, den, dreal, tiles, C)
    switch (D) {
        case 64: SVA_CM(4); break;
        case 128: SVA_CM(8); break;
        case 192: SVA_CM(12); break;
        case 256: SVA_CM(16); break;
        default: return hipErrorInvalidValue;
    }
#undef SVA_CM
    return hipGetLastError();
}

}  // namespace sva
