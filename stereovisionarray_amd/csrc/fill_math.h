// fill_math.h -- the hole filling's rule and the line
// arithmetic of its scan (§4.23) as plain C++ shared by the kernels (fill.hip),
// the argument checks (sva_api.cpp, array_args.h) and the host test program
// (tests/test_fill_cpu.py).  No HIP header.
//
// A pixel is valid iff d != invalid and d != 0 (cc::valid); every other pixel is
// a hole.  Direction k of a hole p looks along p + j * r_k, j = 1..max_dist,
// inside the frame, for the first valid pixel of the INPUT map: its candidate
// (d, j, k), as one integer the key d << 11 | j << 3 | k.  The candidates sorted
// by key, `mode` picks one; fewer than min_found candidates leave the hole.
#pragma once

#include <cstdint>

#include "cross_check_math.h"

#if defined(__clang__)
#define SVA_FL_UNROLL _Pragma("unroll")
#else
#define SVA_FL_UNROLL
#endif

namespace sva {
namespace fl {

constexpr int kDirs = 8;
constexpr int kMaxDist = 255;              // j fits the key's eight bits
constexpr uint32_t kAbsent = 0xFFFFFFFFu;  // the key of a direction without a candidate
constexpr int kModes = 3;                  // SVA_FILL_MIN, _SECOND, _MEDIAN = 0, 1, 2

// r_k = (dx, dy), k = 0..7: E W S N SE NW SW NE; each component + 1 in two bits.
constexpr uint32_t kDxBits = 2u | 0u << 2 | 1u << 4 | 1u << 6 | 2u << 8 | 0u << 10 | 0u << 12 | 2u << 14;
constexpr uint32_t kDyBits = 1u | 1u << 2 | 2u << 4 | 0u << 6 | 2u << 8 | 0u << 10 | 2u << 12 | 0u << 14;
SVA_CC_HD constexpr int dir_dx(int k) { return (int)((kDxBits >> (2 * k)) & 3u) - 1; }
SVA_CC_HD constexpr int dir_dy(int k) { return (int)((kDyBits >> (2 * k)) & 3u) - 1; }
static_assert(dir_dx(0) == 1 && dir_dy(0) == 0 && dir_dx(1) == -1 && dir_dy(1) == 0, "E W");
static_assert(dir_dx(2) == 0 && dir_dy(2) == 1 && dir_dx(3) == 0 && dir_dy(3) == -1, "S N");
static_assert(dir_dx(4) == 1 && dir_dy(4) == 1 && dir_dx(5) == -1 && dir_dy(5) == -1, "SE NW");
static_assert(dir_dx(6) == -1 && dir_dy(6) == 1 && dir_dx(7) == 1 && dir_dy(7) == -1, "SW NE");

// d in 0..65535, j in 1..kMaxDist, k in 0..7: 27 bits, never kAbsent.
SVA_CC_HD constexpr uint32_t make_key(unsigned d, int j, int k) {
    return (uint32_t)d << 11 | (uint32_t)j << 3 | (uint32_t)k;
}
SVA_CC_HD constexpr unsigned key_d(uint32_t key) { return key >> 11; }
SVA_CC_HD constexpr int key_j(uint32_t key) { return (int)(key >> 3 & 255u); }
SVA_CC_HD constexpr int key_k(uint32_t key) { return (int)(key & 7u); }

SVA_CC_HD inline void order(uint32_t& a, uint32_t& b) {
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}

// Eight keys ascending, absent ones last: Batcher's odd-even merge sort, 19
// comparators.  Returns n, the number of keys present.
SVA_CC_HD inline int sort8(uint32_t k[kDirs]) {
    order(k[0], k[1]); order(k[2], k[3]); order(k[4], k[5]); order(k[6], k[7]);
    order(k[0], k[2]); order(k[1], k[3]); order(k[4], k[6]); order(k[5], k[7]);
    order(k[1], k[2]); order(k[5], k[6]);
    order(k[0], k[4]); order(k[1], k[5]); order(k[2], k[6]); order(k[3], k[7]);
    order(k[2], k[4]); order(k[3], k[5]);
    order(k[1], k[2]); order(k[3], k[4]); order(k[5], k[6]);
    int n = 0;
    for (int i = 0; i < kDirs; i++) n += k[i] != kAbsent ? 1 : 0;
    return n;
}

// The index into the sorted keys that `mode` picks among n candidates, or -1
// where n < min_found (min_found >= 1, so n = 0 is always -1).
SVA_CC_HD inline int pick(int n, int min_found, int mode) {
    if (n < min_found || n < 1) return -1;
    if (mode == 0) return 0;
    if (mode == 1) return n > 1 ? 1 : 0;
    return (n - 1) / 2;
}

// The argument rule sva_fill_holes* and sva_array_depth_filled share: the
// message of the first rule broken, or null.
inline const char* thresholds_error(int max_dist, int min_found, int mode) {
    if (max_dist < 0 || max_dist > kMaxDist) return "fill max_dist must be 0..255";
    if (min_found < 1 || min_found > kDirs) return "fill min_found must be 1..8";
    if (mode < 0 || mode >= kModes) return "fill mode must be 0..2";
    return nullptr;
}

// ---- the scan's lines ---------------------------------------------------------
// Direction k's candidate at p is the last valid pixel met when the line through
// p is walked AGAINST r_k, with the steps since.  The horizontal directions
// walk rows: line = y, step t = the t-th pixel of the walk.  The others walk
// rows of the frame top to bottom (S, SE, SW look down, so they are walked
// bottom to top): line = the column at step 0, and a diagonal moves one column
// per step and wraps round the frame's edge (x = (line -+ t) mod W), where a
// new line of the image begins -- so the `lines` threads of one step touch one
// whole row of the map and of the key plane.
SVA_CC_HD inline int n_lines(int k, int W, int H) { return dir_dy(k) == 0 ? H : W; }
SVA_CC_HD inline int n_steps(int k, int W, int H) { return dir_dy(k) == 0 ? W : H; }
// ceil(n_steps / S)
SVA_CC_HD inline int n_segments(int k, int W, int H, int S) {
    return (n_steps(k, W, H) + S - 1) / S;
}

// The walk of segment `seg` (steps seg * S .. min(n_steps, (seg + 1) * S) - 1)
// of line `line`, begun max_dist steps early so that nothing is carried from one
// segment into the next: a candidate lies at most max_dist steps back.
// load(x, y) is the input map's pixel, store(x, y, key) takes direction k's key
// at every pixel of the segment itself.  RING pixels are loaded ahead of the
// dependent chain.  S >= 1, max_dist in 1..kMaxDist, seg < n_segments.
template <int RING, class Load, class Store>
SVA_CC_HD inline void scan_segment(int k, int line, int seg, int W, int H, int S, int max_dist,
                                   unsigned invalid, Load load, Store store) {
    const int steps = n_steps(k, W, H);
    const int wdx = -dir_dx(k), wdy = -dir_dy(k);
    const int t_begin = seg * S;
    const int t_end = steps - t_begin < S ? steps : t_begin + S;
    int t = t_begin > max_dist ? t_begin - max_dist : 0;
    int x, y;
    if (wdy == 0) {
        y = line;
        x = wdx > 0 ? t : W - 1 - t;
    } else {
        y = wdy > 0 ? t : H - 1 - t;
        x = (line + wdx * (t % W)) % W;
        if (x < 0) x += W;
    }
    unsigned d = 0;
    int j = kMaxDist + 1;   // nothing within reach
    bool fresh = true;      // the pixel starts a line of the image (or the walk)
    while (t < t_end) {
        int xs[RING], ys[RING];
        bool fr[RING];
        unsigned v[RING];
        const int n = t_end - t < RING ? t_end - t : RING;
        SVA_FL_UNROLL
        for (int r = 0; r < RING; r++) {
            xs[r] = x;
            ys[r] = y;
            fr[r] = fresh;
            v[r] = r < n ? load(x, y) : 0u;
            // the next pixel of the walk; r >= n - 1 may leave the frame, unused
            x += wdx;
            y += wdy;
            fresh = false;
            if (wdy != 0 && x >= W) {
                x = 0;
                fresh = true;
            } else if (wdy != 0 && x < 0) {
                x = W - 1;
                fresh = true;
            }
        }
        SVA_FL_UNROLL
        for (int r = 0; r < RING; r++) {
            if (r < n) {
                if (fr[r]) j = kMaxDist + 1;
                else if (j <= kMaxDist) j++;
                if (t + r >= t_begin)
                    store(xs[r], ys[r], j <= max_dist ? make_key(d, j, k) : kAbsent);
                if (cc::valid(v[r], invalid)) {
                    d = v[r];
                    j = 0;
                }
            }
        }
        t += n;
        if (n < RING) break;
    }
}

}  // namespace fl
}  // namespace sva
