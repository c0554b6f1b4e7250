// refine.hip -- SURVEY.md §8f rows 1-2 on the GPU: disparity refinement
// (improveWithDisparity + shiftPerspectiveWithDisparity, functions.cpp:11-72)
// and depth <-> 3-D output (shiftPerspective2, Points3DToDepthMap,
// DepthMapToPoints3D, functions.cpp:74-146).  Semantics of the reference's
// undefined corners: DESIGN.md §2.7 (same as oracle/refine_oracle.c).
//
//   shift_perspective_kernel  1 thread/pixel gather (u8), f64 index math
//   refine_box_kernel          1 <= k <= 16: the 11 window SADs as 2k x 2k box
//                              sums of offset AD planes (wave per column strip)
//   refine_kernel<ND>          k = 0, and k <= 16 on planes of 2^31 bytes or more:
//                              1 thread/pixel, 11 candidate SADs on
//                              dword-realigned rows (v_alignbyte + v_sad_u8),
//                              first-minimum, (uchar)(int) of the f64 update
//   refine_sat_*_kernel        k >= 17: the 11 window SADs as four corners of
//                              summed-area tables of the AD planes, work per
//                              pixel independent of k (the box-sum route)
//   scatter_key_kernel /       "last write in loop order wins" scatters as two
//   scatter_write_kernel       passes: atomicMax of (loop index + 1) per target,
//                              then the owner of the winning index writes
//   d2p_count / d2p_scan /     column-major stream compaction (depth > 0.1):
//   d2p_write                  per-(column, 64-row chunk) counts, one-block
//                              exclusive scan, ordered writes
// All f64 in the reference's operand order, no contraction.
#include "sva_device.h"
#include "sva_internal.h"

#pragma clang fp contract(off)

namespace sva {
namespace {

struct CamD {
    double f, px, py, pz, ps;
};
inline CamD camd(const sva_camera& c) { return CamD{c.f, c.pos[0], c.pos[1], c.pos[2], c.pixel_size}; }

// double -> int with the skip rule: false for NaN / outside int range.
__device__ __forceinline__ bool to_int(double v, long long& out) {
    if (!(v > -2147483649.0 && v < 2147483648.0)) return false;
    out = (long long)(int)v;
    return true;
}

__global__ void shift_perspective_kernel(const uint8_t* __restrict__ disp,
                                         const uint8_t* __restrict__ img, int W, int H,
                                         size_t pitch, double preX, double preY,
                                         uint8_t* __restrict__ out, int zero_fill) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const double d = disp[(size_t)y * pitch + x];
    long long sx, sy;
    if (d == 0 || !to_int(d * preX + x, sx) || !to_int(d * preY + y, sy) || sy >= H || sy < 0 ||
        sx >= W || sx < 0) {
        if (zero_fill) out[(size_t)y * pitch + x] = 0;   // untouched pixel of a fresh plane
        return;
    }
    out[(size_t)y * pitch + x] = img[(size_t)sy * pitch + sx];
}

template <int ND>
__global__ __launch_bounds__(256) void refine_kernel(
    const uint8_t* __restrict__ disp, const uint8_t* __restrict__ center,
    const uint8_t* __restrict__ shifted, const uint8_t* __restrict__ mask, int W, int H,
    size_t pitch, int k, int ddx, int ddy, uint8_t* __restrict__ out, int* __restrict__ fault) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * pitch + x;
    if (mask && mask[p] == 0) return;
    const bool ok = x - k >= 0 && x + k <= W && y - k >= 0 && y + k <= H &&
                    x - 5 * ddx - k >= 0 && x + 5 * ddx + k <= W &&
                    y - 5 * ddy - k >= 0 && y + 5 * ddy + k <= H;
    if (!ok) {
        atomicOr(fault, 1);
        return;
    }
    int bi = 0;
    if constexpr (ND > 0) {
        const unsigned lastmask = (k & 1) ? 0xffffu : 0xffffffffu;  // 2k % 4 == 2 -> 2 bytes
        const uint8_t* win = center + (size_t)(y - k) * pitch + (x - k);
        unsigned best = 0;
        for (int c = 0; c <= 10; c++) {
            const int nx = x + ddx * (c - 5), ny = y + ddy * (c - 5);
            const uint8_t* sw = shifted + (size_t)(ny - k) * pitch + (nx - k);
            unsigned acc = 0;
            for (int v = 0; v < 2 * k; v++)
                acc = sad_row<ND>(sw + (size_t)v * pitch, win + (size_t)v * pitch, lastmask, 2 * k,
                                  acc);
            if (c == 0 || acc < best) { best = acc; bi = c; }
        }
    }
    const double v = (double)disp[p] + (double)(bi - 5) * (double)(ddx + ddy);
    out[p] = (uint8_t)(int)v;
}

// Inclusive wave64 scan in 6 DPP adds (row_shr 1/2/4/8, row_bcast 15/31).
__device__ __forceinline__ unsigned wave_scan_incl(unsigned v) {
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
    return v;
}

// Box-filter form of refine_kernel for 1 <= k <= REF_BOX_KMAX.  Candidate c's
// window SAD is the 2k x 2k box sum of the offset plane
// AD_c(q) = |shifted(q + (c-5)*dd) - center(q)|.  A block of 4 waves owns a
// strip of 64 columns x REF_BOX_TH output rows (lane = column x0 - k + lane,
// 65 - 2k outputs per row); wave w takes candidates 3w..3w+2 (the last wave
// repeats 10).  Per AD row and candidate: one AD, a sliding column sum (old AD
// rows packed 3 per dword in an LDS ring of 2k rows), a DPP wave prefix scan
// and one bpermute, SAD(x) = P[lane + 2k - 1] - P[lane - 1].  Each wave folds
// (SAD << 4) | c into an LDS min per output -- the minimum key is the
// first-minimum candidate -- and after one barrier the block writes the
// masked outputs.  Integer-exact.
constexpr int REF_BOX_KMAX = 16, REF_BOX_TH = 32;

typedef __amdgpu_buffer_rsrc_t rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes,
                                             0x00020000);
}

size_t refine_box_lds(int k) { return (size_t)(REF_BOX_TH * 64 + 4 * 2 * k * 64) * 4; }

__global__ __launch_bounds__(256) void refine_box_kernel(
    const uint8_t* __restrict__ disp, const uint8_t* __restrict__ center,
    const uint8_t* __restrict__ shifted, const uint8_t* __restrict__ mask, int W, int H,
    size_t pitch, int k, int ddx, int ddy, uint8_t* __restrict__ out, int* __restrict__ fault) {
    extern __shared__ unsigned smem[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int w2 = 2 * k, OW = 65 - w2;
    const int x0 = blockIdx.x * OW, y0 = blockIdx.y * REF_BOX_TH;
    const int q = x0 - k + lane;
    const int ylim = min(y0 + REF_BOX_TH, H);
    const int rbeg = y0 - k, rend = ylim - 1 + k;    // AD rows [rbeg, rend)
    unsigned* keys = smem;                            // [REF_BOX_TH][64]
    unsigned* ring = smem + REF_BOX_TH * 64 + wv * w2 * 64;

    if (mask) {             // nothing to do for a strip with no masked output pixel
        const int x = x0 + lane;
        // wave w checks rows y0 + w, y0 + w + 4, ... (8 independent loads per lane)
        int any = 0;
        const int xc = min(x, W - 1);
#pragma unroll
        for (int j = 0; j < REF_BOX_TH / 4; j++) {
            const int y = min(y0 + wv + 4 * j, H - 1);
            any |= mask[(size_t)y * pitch + xc];
        }
        if (!__syncthreads_or(any && lane < OW && x < W)) return;
    }
    for (int i = threadIdx.x; i < REF_BOX_TH * 64; i += 256) keys[i] = ~0u;
    __syncthreads();

    // Raw buffer loads, unconditional, used as loaded: offsets before the plane
    // wrap to huge unsigned values and offsets past it read 0 (hardware range
    // check); a column outside [0, W) may read a neighbouring row's byte, but a
    // pixel that passes the window check below only sums in-image positions, so
    // such values never reach an output.  (Guarded loads become exec branches,
    // and the compiler then waits for every load in flight, the prefetch too.)
    // Offsets in wrapping unsigned arithmetic; H * pitch < 2^31 at launch.
    const unsigned plane = (unsigned)((size_t)H * pitch);
    const rsrc_t rc = make_rsrc(center, plane), rsh = make_rsrc(shifted, plane);
    const unsigned st = (unsigned)ddy * (unsigned)pitch + (unsigned)ddx;   // candidate step
    int cand[3];
    unsigned soff[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        cand[j] = min(3 * wv + j, 10);
        soff[j] = (unsigned)(cand[j] - 5) * st;
    }
    struct Row {
        unsigned cb, sb[3];
    };
    auto fetch = [&](int r, Row& n) {
        const unsigned ro = (unsigned)r * (unsigned)pitch + (unsigned)q;
        n.cb = __builtin_amdgcn_raw_buffer_load_b8(rc, ro, 0, 0);
#pragma unroll
        for (int j = 0; j < 3; j++) n.sb[j] = __builtin_amdgcn_raw_buffer_load_b8(rsh, ro + soff[j], 0, 0);
    };
    unsigned col[3] = {0u, 0u, 0u};
    int slot = 0;
    // One AD row: consume cur; the row after next is requested into nxt.
    auto step = [&](int r, const Row& cur, Row& nxt) {
        fetch(r + 2, nxt);
        const int i = r - rbeg;
        unsigned* rs = ring + slot * 64 + lane;
        const unsigned old = i >= w2 ? *rs : 0u;
        unsigned pk = 0;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const unsigned ad = __builtin_amdgcn_sad_u8(cur.cb, cur.sb[j], 0u);
            col[j] = col[j] + ad - ((old >> (8 * j)) & 0xffu);
            pk |= ad << (8 * j);
        }
        *rs = pk;
        if (++slot == w2) slot = 0;
        if (i < w2 - 1) return;
        unsigned key = ~0u;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const unsigned P = wave_scan_incl(col[j]);
            const unsigned hi =
                (unsigned)__builtin_amdgcn_ds_bpermute((lane + w2 - 1) << 2, (int)P);
            key = min(key, ((hi - (P - col[j])) << 4) | (unsigned)cand[j]);
        }
        atomicMin(keys + (r - k + 1 - y0) * 64 + lane, key);
    };
    // Two rows in flight, unrolled by three over rotating row buffers: no
    // register copies of in-flight loads (a copy at the loop end makes the
    // compiler wait for the prefetch).
    Row A, B, C;
    fetch(rbeg, A);
    fetch(rbeg + 1, B);
    for (int r = rbeg; r < rend; r += 3) {
        step(r, A, C);
        if (r + 1 >= rend) break;
        step(r + 1, B, A);
        if (r + 2 >= rend) break;
        step(r + 2, C, B);
    }
    __syncthreads();
    // write-out: all mask / disparity bytes requested before any is used
    const int xo = x0 + lane, xoc = min(xo, W - 1);
    unsigned mv[REF_BOX_TH / 4], dv[REF_BOX_TH / 4];
#pragma unroll
    for (int j = 0; j < REF_BOX_TH / 4; j++) {
        const size_t p = (size_t)min(y0 + wv + 4 * j, H - 1) * pitch + xoc;
        mv[j] = mask ? mask[p] : 1u;
        dv[j] = disp[p];
    }
    if (lane >= OW || xo >= W) return;
#pragma unroll
    for (int j = 0; j < REF_BOX_TH / 4; j++) {
        const int y = y0 + wv + 4 * j, x = xo;
        if (y >= ylim || mv[j] == 0) continue;
        const bool ok = x - k >= 0 && x + k <= W && y - k >= 0 && y + k <= H &&
                        x - 5 * ddx - k >= 0 && x + 5 * ddx + k <= W &&
                        y - 5 * ddy - k >= 0 && y + 5 * ddy + k <= H;
        if (!ok) {
            atomicOr(fault, 1);
            continue;
        }
        const int bi = (int)(keys[(y - y0) * 64 + lane] & 15u);
        const double v = (double)dv[j] + (double)(bi - 5) * (double)(ddx + ddy);
        out[(size_t)y * pitch + x] = (uint8_t)(int)v;
    }
}

// ---- box-sum route: any k, work per pixel and candidate independent of k ------
// Candidate c's window SAD is a box sum of the offset plane AD_c (above), read
// as four corners of AD_c's summed-area table
//   T_c(i, j) = sum of AD_c(x', y') over x' < i, y' < j      (exclusive, so
//   SAD_c(x, y) = T(x+k, y+k) - T(x-k, y+k) - T(x+k, y-k) + T(x-k, y-k)).
// Only the part of the table that some written pixel needs is built: the
// pixels that pass the mask and the window test have a bounding box
// bb = [x0, x1] x [y0, y1] (refine_sat_init_kernel / refine_sat_bbox_kernel,
// which also raise the fault flag), their windows cover the AD columns
// [x0-k, x1+k) and rows [y0-k, y1+k), and every AD there reads in-image
// bytes of both planes because bb lies inside the window-test region
// [k+5ddx, W-k-5ddx] x [k+5ddy, H-k-5ddy].  Sums start at the region's corner.
//   refine_sat_row_kernel   block = one AD row of one candidate: exclusive row
//                           prefix in rounds of 1024 columns with a carry
//   refine_sat_col_kernel   lane = one table column of one candidate: running
//                           sum down the rows, in place
//   refine_sat_pick_kernel  thread = pixel: the candidates' four corners, plain
//                           (sum, c) compare with strict <, first minimum
// Tables are [H+1][W+1] per candidate, addressed in size_t.  S = u32 holds the
// table modulo 2^32, which gives the exact SAD while (2k)^2 * 255 < 2^32
// (k <= 2052); from k = 2053 S = u64.  Candidates run in groups of as many
// tables as the workspace holds; between groups the running (sum, c) of each
// pixel waits in best_s / best_c.
constexpr int REF_SAT_ROUND = 1024, REF_SAT_BBOX_ROWS = 16, REF_SAT_KWIDE = 2053;
constexpr size_t REF_SAT_HEAD = 256;                      // bb lives in front of the tables
constexpr size_t REF_SAT_TABLE_BYTES = (size_t)512 << 20;  // group size: tables within this

__global__ void refine_sat_init_kernel(int* __restrict__ bb, int xlo, int xhi, int ylo, int yhi,
                                       int nomask, int* __restrict__ fault) {
    if (nomask) {
        // every pixel is masked: bb is the window-test region, and since k >= 1
        // the frame's border pixels fail the test
        bb[0] = xlo; bb[1] = xhi; bb[2] = ylo; bb[3] = yhi;
        atomicOr(fault, 1);
    } else {
        bb[0] = 0x7fffffff; bb[1] = -1; bb[2] = 0x7fffffff; bb[3] = -1;
    }
}

// bb = bounding box of the masked pixels inside [xlo, xhi] x [ylo, yhi]; a
// masked pixel outside raises the fault flag.  Thread = column, 16 rows each.
__global__ __launch_bounds__(256) void refine_sat_bbox_kernel(
    const uint8_t* __restrict__ mask, int W, int H, size_t pitch, int xlo, int xhi, int ylo,
    int yhi, int* __restrict__ bb, int* __restrict__ fault) {
    const int lane = threadIdx.x & 63;
    const int x = blockIdx.x * 256 + threadIdx.x, yb = blockIdx.y * REF_SAT_BBOX_ROWS;
    int ymin = 0x7fffffff, ymax = -1, bad = 0;
    if (x < W) {
        const bool xin = x >= xlo && x <= xhi;
        for (int j = 0; j < REF_SAT_BBOX_ROWS; j++) {
            const int y = yb + j;
            if (y >= H) break;
            if (mask[(size_t)y * pitch + x] == 0) continue;
            if (xin && y >= ylo && y <= yhi) {
                ymin = min(ymin, y);
                ymax = max(ymax, y);
            } else {
                bad = 1;
            }
        }
    }
    if (__any(bad) && lane == 0) atomicOr(fault, 1);
    const unsigned long long hit = __ballot(ymax >= 0);
    if (!hit) return;
    for (int o = 32; o >= 1; o >>= 1) {
        ymin = min(ymin, __shfl_xor(ymin, o));
        ymax = max(ymax, __shfl_xor(ymax, o));
    }
    if (lane == 0) {
        atomicMin(bb + 0, x + __ffsll(hit) - 1);
        atomicMax(bb + 1, x + 63 - __clzll(hit));
        atomicMin(bb + 2, ymin);
        atomicMax(bb + 3, ymax);
    }
}

template <typename S>
__global__ __launch_bounds__(REF_SAT_ROUND) void refine_sat_row_kernel(
    const uint8_t* __restrict__ center, const uint8_t* __restrict__ shifted, int W, int H,
    size_t pitch, int k, int ddx, int ddy, int cbeg, const int* __restrict__ bb,
    S* __restrict__ sat) {
    __shared__ unsigned wsum[2][REF_SAT_ROUND / 64];
    const int x0 = bb[0], x1 = bb[1], y0 = bb[2], y1 = bb[3];
    if (x0 > x1) return;
    const int qy = blockIdx.x;                       // AD row
    if (qy < y0 - k || qy >= y1 + k) return;
    const int rx0 = x0 - k, n = x1 - x0 + 2 * k;     // AD columns rx0 .. rx0 + n - 1
    const int c = cbeg + blockIdx.y;
    const uint8_t* crow = center + (size_t)qy * pitch;
    const uint8_t* srow = shifted + (size_t)(qy + (c - 5) * ddy) * pitch;
    const int sx = (c - 5) * ddx;
    S* row = sat + (size_t)blockIdx.y * ((size_t)(W + 1) * (size_t)(H + 1)) +
             (size_t)(qy + 1) * (size_t)(W + 1);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    S carry = 0;
    // n + 1 prefix entries; rounds alternate between the two wsum rows, so one
    // barrier per round orders both the wave totals and their reuse
    for (int base = 0, r = 0; base <= n; base += REF_SAT_ROUND, r ^= 1) {
        const int i = base + t;
        unsigned ad = 0;
        if (i < n) {
            const int qx = rx0 + i;
            ad = __builtin_amdgcn_sad_u8((unsigned)crow[qx], (unsigned)srow[qx + sx], 0u);
        }
        const unsigned incl = wave_scan_incl(ad);
        if (lane == 63) wsum[r][wave] = incl;
        __syncthreads();
        unsigned before = 0, round = 0;
#pragma unroll
        for (int w = 0; w < REF_SAT_ROUND / 64; w++) {
            const unsigned ws = wsum[r][w];
            if (w < wave) before += ws;
            round += ws;
        }
        if (i <= n) row[rx0 + i] = carry + (S)(before + incl - ad);
        carry += (S)round;
    }
}

template <typename S>
__global__ __launch_bounds__(64) void refine_sat_col_kernel(int W, int H, int k,
                                                            const int* __restrict__ bb,
                                                            S* __restrict__ sat) {
    const int x0 = bb[0], x1 = bb[1], y0 = bb[2], y1 = bb[3];
    if (x0 > x1) return;
    const int qx = blockIdx.x * 64 + threadIdx.x;    // table column
    if (qx < x0 - k || qx > x1 + k) return;
    const size_t ps = (size_t)(W + 1);
    const int r0 = y0 - k, r1 = y1 + k;              // AD rows [r0, r1), table rows r0 .. r1
    S* p = sat + (size_t)blockIdx.y * (ps * (size_t)(H + 1)) + (size_t)r0 * ps + qx;
    *p = 0;
    p += ps;
    S acc = 0;
    int r = r0;
    for (; r + 8 <= r1; r += 8, p += 8 * ps) {       // eight rows requested before any is used
        S v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = p[(size_t)u * ps];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            acc += v[u];
            p[(size_t)u * ps] = acc;
        }
    }
    for (; r < r1; r++, p += ps) {
        acc += *p;
        *p = acc;
    }
}

template <typename S>
__global__ __launch_bounds__(256) void refine_sat_pick_kernel(
    const uint8_t* __restrict__ disp, const uint8_t* __restrict__ mask, int W, int H,
    size_t pitch, int k, int ddx, int ddy, int xlo, int ylo, int cbeg, int cend,
    const int* __restrict__ bb, const S* __restrict__ sat, unsigned long long* __restrict__ best_s,
    uint8_t* __restrict__ best_c, uint8_t* __restrict__ out) {
    const int x = xlo + blockIdx.x * 64 + threadIdx.x, y = ylo + blockIdx.y * 4 + threadIdx.y;
    if (x < bb[0] || x > bb[1] || y < bb[2] || y > bb[3]) return;
    const size_t p = (size_t)y * pitch + x;
    if (mask && mask[p] == 0) return;
    const size_t ps = (size_t)(W + 1), plane = ps * (size_t)(H + 1), si = (size_t)y * W + x;
    S best = 0;
    int bi = 0;
    if (cbeg > 0) {
        best = (S)best_s[si];
        bi = best_c[si];
    }
    const S* a = sat + (size_t)(y - k) * ps + (x - k);
    const size_t dn = (size_t)(2 * k) * ps;
    for (int c = cbeg; c < cend; c++, a += plane) {
        const S e = (a[dn + 2 * k] - a[dn]) - (a[2 * k] - a[0]);
        if (c == 0 || e < best) { best = e; bi = c; }
    }
    if (cend <= 10) {
        best_s[si] = best;
        best_c[si] = (uint8_t)bi;
        return;
    }
    const double v = (double)disp[p] + (double)(bi - 5) * (double)(ddx + ddy);
    out[p] = (uint8_t)(int)v;
}

// ---- scatters: last write in loop order wins --------------------------------
// Source s (loop index) writes target t: pass 1 keys[t] = max(idx + 1), pass 2
// the source whose idx + 1 equals keys[t] writes its value.

struct Shift2 {
    double preX, preY;
};

__device__ __forceinline__ bool shift2_target(const Shift2& g, double d, int x, int y, int W,
                                              int H, unsigned& t) {
    if (d < 0.5) return false;
    long long tx, ty;
    if (!to_int(g.preX / d, tx) || !to_int(g.preY / d, ty)) return false;
    const long long sx = tx + x, sy = ty + y;
    if (sy >= H || sy < 0 || sx >= W || sx < 0) return false;
    t = (unsigned)(sy * W + sx);
    return true;
}

__global__ void shift2_kernel(const double* __restrict__ depth, int W, int H, Shift2 g,
                              unsigned* __restrict__ keys, double* __restrict__ out, int pass) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const double d = depth[(size_t)y * W + x];
    unsigned t;
    if (!shift2_target(g, d, x, y, W, H, t)) return;
    const unsigned key = (unsigned)x * (unsigned)H + (unsigned)y + 1u;   // x-major loop order
    if (pass == 0) atomicMax(keys + t, key);
    else if (keys[t] == key) out[t] = d;
}

__device__ __forceinline__ bool project_target(const CamD& c, const double* P, int W, int H,
                                               unsigned& t) {
    const double mult = c.f / (P[2] - c.pz) / c.ps;
    long long px, py;
    if (!to_int((P[0] - c.px) * mult, px) || !to_int((P[1] - c.py) * mult, py)) return false;
    px += W / 2;
    py += H / 2;
    if (!(px >= 0 && px < W && py >= 0 && py < H)) return false;
    t = (unsigned)(py * W + px);
    return true;
}

__global__ void points_to_depth_kernel(const double* __restrict__ pts, long long n, CamD c, int W,
                                       int H, unsigned* __restrict__ keys,
                                       double* __restrict__ out, int pass) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double P[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    unsigned t;
    if (!project_target(c, P, W, H, t)) return;
    const unsigned key = (unsigned)i + 1u;
    if (pass == 0) atomicMax(keys + t, key);
    else if (keys[t] == key) out[t] = P[2] - c.pz;
}

// ---- DepthMapToPoints3D: ordered compaction ----------------------------------
constexpr int D2P_ROWS = 64;

__global__ void d2p_count_kernel(const double* __restrict__ depth, int W, int H, int nch,
                                 unsigned* __restrict__ counts) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x, ch = blockIdx.y;
    if (u >= W) return;
    const int v0 = ch * D2P_ROWS, v1 = min(H, v0 + D2P_ROWS);
    unsigned n = 0;
    for (int v = v0; v < v1; v++) n += depth[(size_t)v * W + u] > 0.1;
    counts[(size_t)u * nch + ch] = n;   // column-major unit order
}

// One block: exclusive scan of counts[0..n) in place; total -> *total.
// Rounds of 1024 consecutive counts (one coalesced load per thread), a DPP
// wave scan, the 16 wave totals combined through LDS, and a running carry.
// (A per-thread walk over 32 contiguous counts serialised the loads: 58 us.)
__global__ __launch_bounds__(1024) void d2p_scan_kernel(unsigned* __restrict__ counts, int n,
                                                       long long* __restrict__ total) {
    __shared__ unsigned wsum[16];
    __shared__ unsigned long long carry_s;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < n; base += 1024) {
        const int i = base + t;
        const unsigned c = i < n ? counts[i] : 0u;
        const unsigned incl = wave_scan_incl(c);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned before = 0, round = 0;
        for (int w = 0; w < 16; w++) {
            const unsigned ws = wsum[w];
            if (w < wave) before += ws;
            round += ws;
        }
        const unsigned long long carry = carry_s;
        if (i < n) counts[i] = (unsigned)(carry + before + incl - c);
        __syncthreads();                      // everyone has read wsum / carry_s
        if (t == 0) carry_s = carry + round;
        __syncthreads();
    }
    if (t == 0) *total = (long long)carry_s;
}

__global__ void d2p_write_kernel(const double* __restrict__ depth, int W, int H, int nch,
                                 const unsigned* __restrict__ offs, CamD c,
                                 double* __restrict__ pts) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x, ch = blockIdx.y;
    if (u >= W) return;
    const int v0 = ch * D2P_ROWS, v1 = min(H, v0 + D2P_ROWS);
    size_t o = offs[(size_t)u * nch + ch];
    const double r0 = (double)(u - W / 2) * c.ps;
    for (int v = v0; v < v1; v++) {
        const double d = depth[(size_t)v * W + u];
        if (!(d > 0.1)) continue;
        // Camera::inv_project (Camera.cpp:25-33), then pos3D + r * depth
        const double r1 = (double)(v - H / 2) * c.ps, r2 = c.f;
        const double nrm = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
        pts[3 * o + 0] = c.px + (r0 / nrm) * d;
        pts[3 * o + 1] = c.py + (r1 / nrm) * d;
        pts[3 * o + 2] = c.pz + (r2 / nrm) * d;
        o++;
    }
}

}  // namespace

hipError_t launch_shift_perspective(Ctx& c, const sva_camera& in, const sva_camera& out,
                                    const uint8_t* disp, const uint8_t* img, int W, int H,
                                    size_t pitch, uint8_t* shifted, bool zero_fill) {
    ScopedKernelTimer t(c, "shift_perspective");
    // preMult (functions.cpp:56-57): (in - out) / norm(in - out), host f64, no contraction
    const double dx = in.pos[0] - out.pos[0], dy = in.pos[1] - out.pos[1],
                 dz = in.pos[2] - out.pos[2];
    const double n = sqrt(dx * dx + dy * dy + dz * dz);
    hipLaunchKernelGGL(shift_perspective_kernel, dim3((W + 255) / 256, H), dim3(256), 0, c.stream,
                       disp, img, W, H, pitch, dx / n, dy / n, shifted, (int)zero_fill);
    return hipGetLastError();
}

// Candidate tables per group and the workspace they need (include/sva.h states
// the same formula).
struct SatPlan {
    size_t table;    // bytes of one candidate's table
    int group;       // tables resident at once, 1..11
    size_t state;    // offset of best_s / best_c (groups < 11 only)
    size_t bytes;    // whole workspace
};
SatPlan sat_plan(int W, int H, int k) {
    SatPlan p;
    p.table = (size_t)(k >= REF_SAT_KWIDE ? 8 : 4) * (size_t)(W + 1) * (size_t)(H + 1);
    const size_t fit = REF_SAT_TABLE_BYTES / p.table;
    p.group = fit >= 11 ? 11 : fit >= 1 ? (int)fit : 1;
    p.state = (REF_SAT_HEAD + (size_t)p.group * p.table + 7) & ~(size_t)7;
    p.bytes = p.state + (p.group < 11 ? (size_t)9 * W * H : 0);
    return p;
}

template <typename S>
void launch_sat_passes(Ctx& c, const uint8_t* disp, const uint8_t* center, const uint8_t* shifted,
                       const uint8_t* mask, int W, int H, size_t pitch, int k, int ddx, int ddy,
                       int xlo, int xhi, int ylo, int yhi, const SatPlan& pl, uint8_t* out) {
    uint8_t* ws = (uint8_t*)c.refine_ws.ptr;
    const int* bb = (const int*)ws;
    S* sat = (S*)(ws + REF_SAT_HEAD);
    unsigned long long* best_s = (unsigned long long*)(ws + pl.state);
    uint8_t* best_c = (uint8_t*)(best_s + (size_t)W * H);
    const dim3 pick_grid((xhi - xlo) / 64 + 1, (yhi - ylo) / 4 + 1);
    for (int cbeg = 0; cbeg < 11; cbeg += pl.group) {
        const int ng = pl.group < 11 - cbeg ? pl.group : 11 - cbeg;
        hipLaunchKernelGGL(refine_sat_row_kernel<S>, dim3(H, ng), dim3(REF_SAT_ROUND), 0, c.stream,
                           center, shifted, W, H, pitch, k, ddx, ddy, cbeg, bb, sat);
        hipLaunchKernelGGL(refine_sat_col_kernel<S>, dim3(W / 64 + 1, ng), dim3(64), 0, c.stream, W,
                           H, k, bb, sat);
        hipLaunchKernelGGL(refine_sat_pick_kernel<S>, pick_grid, dim3(64, 4), 0, c.stream, disp,
                           mask, W, H, pitch, k, ddx, ddy, xlo, ylo, cbeg, cbeg + ng, bb,
                           (const S*)sat, best_s, best_c, out);
    }
}

// The box-sum route, k >= 1.  A window that cannot fit (2k + 10 ddx > W or
// 2k + 10 ddy > H, in 64-bit so that any window_size is safe) writes nothing:
// only the mask decides the fault flag.
hipError_t launch_refine_sat(Ctx& c, const uint8_t* disp, const uint8_t* center,
                             const uint8_t* shifted, const uint8_t* mask, int W, int H,
                             size_t pitch, int k, int ddx, int ddy, uint8_t* out, int* fault) {
    const long long xl = (long long)k + 5 * ddx, xh = (long long)W - k - 5 * ddx;
    const long long yl = (long long)k + 5 * ddy, yh = (long long)H - k - 5 * ddy;
    const bool fits = xl <= xh && yl <= yh;
    const int xlo = fits ? (int)xl : 1, xhi = fits ? (int)xh : 0;
    const int ylo = fits ? (int)yl : 1, yhi = fits ? (int)yh : 0;
    const SatPlan pl = fits ? sat_plan(W, H, k) : SatPlan{0, 0, REF_SAT_HEAD, REF_SAT_HEAD};
    hipError_t e = c.refine_ws.ensure(pl.bytes);
    if (e != hipSuccess) return e;
    int* bb = (int*)c.refine_ws.ptr;
    hipLaunchKernelGGL(refine_sat_init_kernel, dim3(1), dim3(1), 0, c.stream, bb, xlo, xhi, ylo, yhi,
                       mask ? 0 : 1, fault);
    if (mask)
        hipLaunchKernelGGL(refine_sat_bbox_kernel,
                           dim3((W + 255) / 256, (H + REF_SAT_BBOX_ROWS - 1) / REF_SAT_BBOX_ROWS),
                           dim3(256), 0, c.stream, mask, W, H, pitch, xlo, xhi, ylo, yhi, bb, fault);
    if (fits) {
        if (k >= REF_SAT_KWIDE)
            launch_sat_passes<unsigned long long>(c, disp, center, shifted, mask, W, H, pitch, k,
                                                  ddx, ddy, xlo, xhi, ylo, yhi, pl, out);
        else
            launch_sat_passes<unsigned>(c, disp, center, shifted, mask, W, H, pitch, k, ddx, ddy,
                                        xlo, xhi, ylo, yhi, pl, out);
    }
    return hipGetLastError();
}

hipError_t launch_refine(Ctx& c, const uint8_t* disp, const uint8_t* center,
                         const uint8_t* shifted, const uint8_t* mask, int W, int H, size_t pitch,
                         int k, const sva_camera& c0, const sva_camera& c1, uint8_t* out,
                         int* fault) {
    ScopedKernelTimer t(c, "refine");
    // 0/1 direction (functions.cpp:23-25): v / norm(v) && (v > 0.001)
    const int ddx = (c0.pos[0] - c1.pos[0]) > 0.001 ? 1 : 0;
    const int ddy = (c0.pos[1] - c1.pos[1]) > 0.001 ? 1 : 0;
    // k > 16: the box-sum route (SVA_DEBUG_REFINE_ROUTE = 1: every k >= 1).  At
    // k = 17, 24 and 32 it measured 6x to 42x faster than refine_kernel<ND>, with
    // and without a mask; at k = 10 the box kernel is 3x to 4x
    // faster than it.
    if (k > REF_BOX_KMAX || (k >= 1 && c.dbg_refine_route == 1)) {
        c.last_refine_route = 2;
        return launch_refine_sat(c, disp, center, shifted, mask, W, H, pitch, k, ddx, ddy, out,
                                 fault);
    }
    if (k >= 1 && (size_t)H * pitch < ((size_t)1 << 31)) {
        c.last_refine_route = 0;
        const int ow = 65 - 2 * k;
        hipLaunchKernelGGL(refine_box_kernel, dim3((W + ow - 1) / ow, (H + REF_BOX_TH - 1) / REF_BOX_TH),
                           dim3(256), refine_box_lds(k), c.stream, disp, center, shifted, mask, W,
                           H, pitch, k, ddx, ddy, out, fault);
        return hipGetLastError();
    }
    // k = 0, and k <= 16 on planes too large for the box kernel's 32-bit offsets
    c.last_refine_route = 1;
    const dim3 grid((W + 63) / 64, (H + 3) / 4);
    // ND = ceil(2k / 4) = 0..8
    const bool launched = for_int_in<0, 8>((k + 1) / 2, [&](auto ND) {
        hipLaunchKernelGGL(refine_kernel<decltype(ND)::value>, grid, dim3(64, 4), 0, c.stream, disp,
                           center, shifted, mask, W, H, pitch, k, ddx, ddy, out, fault);
    });
    return launched ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_shift_perspective2(Ctx& c, const sva_camera& in, const sva_camera& out,
                                     const double* depth, int W, int H, unsigned* keys,
                                     double* shifted) {
    ScopedKernelTimer t(c, "shift_perspective2");
    // preMult (functions.cpp:77-78): (in - out) * f / pixel_size
    Shift2 g{(in.pos[0] - out.pos[0]) * in.f / in.pixel_size,
             (in.pos[1] - out.pos[1]) * in.f / in.pixel_size};
    hipError_t e = hipMemsetAsync(keys, 0, (size_t)W * H * 4, c.stream);
    if (e != hipSuccess) return e;
    const dim3 grid((W + 255) / 256, H);
    hipLaunchKernelGGL(shift2_kernel, grid, dim3(256), 0, c.stream, depth, W, H, g, keys, shifted, 0);
    hipLaunchKernelGGL(shift2_kernel, grid, dim3(256), 0, c.stream, depth, W, H, g, keys, shifted, 1);
    return hipGetLastError();
}

hipError_t launch_points_to_depth(Ctx& c, const double* pts, long long n, const sva_camera& cam,
                                  int W, int H, unsigned* keys, double* depth) {
    ScopedKernelTimer t(c, "points_to_depth");
    hipError_t e = hipMemsetAsync(keys, 0, (size_t)W * H * 4, c.stream);
    if (e != hipSuccess) return e;
    if (n == 0) return hipSuccess;
    const dim3 grid((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(points_to_depth_kernel, grid, dim3(256), 0, c.stream, pts, n, camd(cam), W,
                       H, keys, depth, 0);
    hipLaunchKernelGGL(points_to_depth_kernel, grid, dim3(256), 0, c.stream, pts, n, camd(cam), W,
                       H, keys, depth, 1);
    return hipGetLastError();
}

size_t d2p_units(int W, int H) { return (size_t)W * ((H + D2P_ROWS - 1) / D2P_ROWS); }

hipError_t launch_depth_to_points(Ctx& c, const double* depth, int W, int H,
                                  const sva_camera& cam, unsigned* counts, long long* total,
                                  double* pts) {
    ScopedKernelTimer t(c, "depth_to_points");
    const int nch = (H + D2P_ROWS - 1) / D2P_ROWS;
    const dim3 grid((W + 255) / 256, nch);
    hipLaunchKernelGGL(d2p_count_kernel, grid, dim3(256), 0, c.stream, depth, W, H, nch, counts);
    hipLaunchKernelGGL(d2p_scan_kernel, dim3(1), dim3(1024), 0, c.stream, counts, W * nch, total);
    hipLaunchKernelGGL(d2p_write_kernel, grid, dim3(256), 0, c.stream, depth, W, H, nch, counts,
                       camd(cam), pts);
    return hipGetLastError();
}

}  // namespace sva
