// wmedian_math.h -- the weighted median filter's rule as plain
// C++ shared by the kernel (wmedian.hip), the argument checks (sva_api.cpp,
// array_args.h) and the host test program (tests/test_wmed_cpu.py).  No HIP
// header.
//
// A pixel is valid iff d != invalid and d != 0 (cc::valid).  The candidates of a
// pixel p are the valid pixels q of its (2r + 1)^2 window inside the frame with
// weight w[|g(p) - g(q)|] > 0 (1 without a guide).  Sorted by (d, qy, qx), the
// pick is the first candidate at which twice the running weight reaches the
// total T: the lower weighted median, with one source pixel.
//
// The window is read through a functor `win`: win.d(i, j) is the STAGED value of
// the cell i columns and j rows from the window's top-left corner (i, j in
// 0..2r) -- the disparity where the cell is a valid pixel of the frame, 0 where
// it is not, so no caller tests a bound -- win.g(i, j) its guide intensity (any
// value where d is 0) and win.w(delta) the table's entry.  The pick is found
// without sorting: one pass for T, n and the value range, a bisection on the
// value (one pass per step: the weight at or below mid) and one pass that walks
// the cells of the median value in raster order.
#pragma once

#include <cstdint>

#include "cross_check_math.h"

namespace sva {
namespace wm {

constexpr int kMaxRadius = 15;
constexpr int kMaxSupport = (2 * kMaxRadius + 1) * (2 * kMaxRadius + 1);   // 961
constexpr int kWeights = 256;
// T <= 961 * 65,535 < 2^26: twice any sum fits 32 bits
static_assert((unsigned long long)kMaxSupport * 65535ull < (1ull << 26), "u32 sums");

// The first rule of {radius, min_support, fill} that fails, in sva.h's order.
SVA_CC_HD inline const char* thresholds_error(int radius, int min_support, int fill) {
    if (radius < 1 || radius > kMaxRadius) return "wmed radius must be 1..15";
    if (min_support < 1 || min_support > kMaxSupport) return "wmed min_support must be 1..961";
    if (fill < 0 || fill > 1) return "wmed fill must be 0 or 1";
    return nullptr;
}

// What a cell is staged as: its disparity, or 0 = "not a candidate".
SVA_CC_HD inline unsigned staged(unsigned d, unsigned invalid) {
    return cc::valid(d, invalid) ? d : 0u;
}

// Does the filter look at pixel p at all?  sel: select[p], or 1 without a plane.
SVA_CC_HD inline bool considered(unsigned sel, int fill, unsigned d, unsigned invalid) {
    return sel != 0u && (fill != 0 || cc::valid(d, invalid));
}

// The weight of the cell (i, j) for a centre of intensity gp; 0: no candidate.
template <bool GUIDED, class Win>
SVA_CC_HD inline unsigned weight(const Win& win, int i, int j, unsigned ds, int gp) {
    if (!GUIDED) return ds != 0u ? 1u : 0u;
    const int delta = gp - (int)win.g(i, j);
    return ds != 0u ? win.w(delta < 0 ? -delta : delta) : 0u;
}

// One bisection step's sum: the weight of the candidates with d <= mid.
template <bool GUIDED, class Win>
SVA_CC_HD inline unsigned weight_at_or_below(const Win& win, int r, int gp, unsigned mid) {
    unsigned s = 0;
    for (int j = 0; j <= 2 * r; j++)
        for (int i = 0; i <= 2 * r; i++) {
            const unsigned ds = win.d(i, j);
            const unsigned w = weight<GUIDED>(win, i, j, ds, gp);
            s += ds <= mid ? w : 0u;
        }
    return s;
}

struct Pick {
    unsigned n;      // the number of candidates
    bool written;    // n >= min_support; d, i, j hold the pick only then
    unsigned d;
    int i, j;        // the source's cell in the window
};

// The pick of one considered pixel.  min_support >= 1.
template <bool GUIDED, class Win>
SVA_CC_HD inline Pick pick(const Win& win, int r, int gp, int min_support) {
    // T, n and the candidates' value range
    unsigned T = 0, n = 0, lo = 0xFFFFFFFFu, hi = 0;
    for (int j = 0; j <= 2 * r; j++)
        for (int i = 0; i <= 2 * r; i++) {
            const unsigned ds = win.d(i, j);
            const unsigned w = weight<GUIDED>(win, i, j, ds, gp);
            const bool c = w != 0u;
            T += w;
            n += c ? 1u : 0u;
            lo = c && ds < lo ? ds : lo;
            hi = c && ds > hi ? ds : hi;
        }
    Pick p{n, n >= (unsigned)min_support, 0u, 0, 0};
    if (!p.written) return p;
    // the least value v with 2 * (weight at or below v) >= T; `below` follows the
    // weight under lo: lo only ever moves to mid + 1, with the sum at mid in hand
    unsigned below = 0;
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo) / 2u;
        const unsigned s = weight_at_or_below<GUIDED>(win, r, gp, mid);
        if (2u * s >= T) {
            hi = mid;
        } else {
            lo = mid + 1u;
            below = s;
        }
    }
    p.d = lo;
    // the tie walk: the cells of that value in raster order; 2 * below < T
    const unsigned need = T - 2u * below;
    unsigned acc = 0;
    bool found = false;
    for (int j = 0; j <= 2 * r; j++)
        for (int i = 0; i <= 2 * r; i++) {
            const unsigned ds = win.d(i, j);
            const unsigned w = ds == lo ? weight<GUIDED>(win, i, j, ds, gp) : 0u;
            acc += w;
            const bool here = !found && w != 0u && 2u * acc >= need;
            p.i = here ? i : p.i;
            p.j = here ? j : p.j;
            found = found || here;
        }
    return p;
}

}  // namespace wm
}  // namespace sva
