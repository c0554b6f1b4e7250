// ref_line.h -- the line arithmetic of Mode R: the reference's
// Bresenham line in closed form, and the interval of one line's offsets that
// the plane kernel tests per outer offset.  Shared by refpath.hip and a host
// test program (tests/test_ref_line_cpu.py checks it against the reference's
// point lists and brute force).  Plain C++: no HIP header on the host side.
#pragma once

#include <cstdlib>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SVA_REF_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SVA_REF_HD inline
#endif

namespace sva {

// Closed form of functions.cpp:253-321.  The line is stored as its start
// point, the major-axis direction and the Bresenham slope numerator/denominator
// so candidate i is O(1):  plotLineLow emits (x0+i, y0 + yi*floor((2|dy|i + dx - 1) / (2dx))),
// plotLineHigh the transpose.  (Proof: the error term D_i = 2|dy|(i+1) - dx -
// 2dx*n_i stays in (-2dx, 2|dy|], which gives n_i = ceil((2|dy|i - dx)/(2dx)).)
struct Line {
    int x0, y0;   // first emitted point
    int high;     // 1: plotLineHigh (y major)
    int step;     // +-1 minor-axis step (yi / xi)
    int a, b;     // 2*|minor delta|, 2*major delta
    int major;    // major delta (dx for low, dy for high)
    int n;        // number of points
};

SVA_REF_HD Line make_line(int p1x, int p1y, int p2x, int p2y) {
    // bresenham(point2 = pixel1, point1 = pixel2), functions.cpp:299-321
    const int ax = p1x, ay = p1y, bx = p2x, by = p2y;
    int x0, y0, x1, y1;
    Line L;
    if (abs(ay - by) < abs(ax - bx)) {
        if (bx > ax) { x0 = ax; y0 = ay; x1 = bx; y1 = by; }
        else { x0 = bx; y0 = by; x1 = ax; y1 = ay; }
        int dx = x1 - x0, dy = y1 - y0;
        L.high = 0;
        L.step = dy < 0 ? -1 : 1;
        L.a = 2 * (dy < 0 ? -dy : dy);
        L.b = 2 * dx;
        L.major = dx;
        L.n = dx + 1;
    } else {
        if (by > ay) { x0 = ax; y0 = ay; x1 = bx; y1 = by; }
        else { x0 = bx; y0 = by; x1 = ax; y1 = ay; }
        int dx = x1 - x0, dy = y1 - y0;
        L.high = 1;
        L.step = dx < 0 ? -1 : 1;
        L.a = 2 * (dx < 0 ? -dx : dx);
        L.b = 2 * dy;
        L.major = dy;
        L.n = dy + 1;   // dy >= 0 here; dy == 0 only for a single point
    }
    L.x0 = x0;
    L.y0 = y0;
    return L;
}

SVA_REF_HD void line_point(const Line& L, int i, int& cx, int& cy) {
    const int minor = L.b > 0 ? (L.a * i + L.major - 1) / L.b : 0;
    if (L.high) { cx = L.x0 + L.step * minor; cy = L.y0 + i; }
    else { cx = L.x0 + i; cy = L.y0 + L.step * minor; }
}

// line_interval's packed arguments, 16-bit halves: up to 32,767 pixels a side
// (sva_api.cpp check_ref_args) offsets and n are within +-32,767, a, b < 65,536.
//   po: a pixel minus its line's start (ox, oy), along the line's major axis
//       (low half, signed) and its minor axis (high half, signed);
//   pa = a | b << 16;  pn = n | major << 16, with n = 0 for a pixel that takes
//       no part (every interval is then empty).
SVA_REF_HD int line_po(int o_major, int o_minor) {
    return (o_major & 0xffff) | (int)((unsigned)o_minor << 16);
}
SVA_REF_HD int line_pa(const Line& L) { return L.a | (int)((unsigned)L.b << 16); }
SVA_REF_HD int line_pn(const Line& L, bool ok) {
    return (ok ? L.n : 0) | (int)((unsigned)L.major << 16);
}

// Interval [lo, lo + len) of inner offsets d_in on a pixel's line at outer
// offset d_out; the candidate index there is i = d_in + ib0.
//   po, pa, pn: line_po, line_pa, line_pn of the pixel and its line;
//   mi: the line's major axis is the inner axis; neg: minor step is -1.
// Candidate i of a line has minor offset floor((a*i + major - 1) / b)
// (make_line's closed form of functions.cpp:253-321).  The int product
// (tt + 1) * b fits for every outer offset while b < 32,768 (frames up to 16,384
// a side), in larger frames for the line's own outer offsets (tt <= major).
SVA_REF_HD void line_interval(int po, int pa, int pn, bool mi, bool neg, int d_out, int& lo,
                              int& len, int& ib0) {
    const int o_major = (int)(short)(po & 0xffff), o_minor = po >> 16;
    const int a = pa & 0xffff, b = (int)((unsigned)pa >> 16);
    const int n = pn & 0xffff, mj = (int)((unsigned)pn >> 16) - 1;
    if (mi) {
        // i = o_major + d_in, and floor((a*i + mj) / b) must equal the
        // candidate's minor offset tt = step * (o_minor + d_out)
        const int u = o_minor + d_out;
        const int tt = neg ? -u : u;
        int ilo = 0, ihi = 0;
        if (tt >= 0) {
            if (a == 0) {
                ihi = tt == 0 ? n : 0;
            } else {
                // i in [ceil((tt*b - mj)/a), ceil((tt*b + b - mj)/a)); the
                // lower bound at tt = 0 is <= 0, i.e. 0 after clamping (the plane
                // kernel's outer loop hoists the reciprocal of a: DESIGN.md §4.2)
                const unsigned A = (unsigned)a;
                ilo = tt == 0 ? 0 : (int)(((unsigned)(tt * b - mj) + A - 1u) / A);
                ihi = (int)(((unsigned)(tt * b + b - mj) + A - 1u) / A);
            }
        }
        ihi = ihi > n ? n : ihi;
        len = ihi > ilo ? ihi - ilo : 0;
        lo = ilo - o_major;
        ib0 = o_major;
    } else {
        // i = o_major + d_out is fixed; one inner offset is on the line
        const int i = o_major + d_out;
        const bool in = (unsigned)i < (unsigned)n;
        const int t = (b > 0 && in) ? (int)((unsigned)(a * i + mj) / (unsigned)b) : 0;
        lo = (neg ? -t : t) - o_minor;
        len = in ? 1 : 0;
        ib0 = i - lo;
    }
}

}  // namespace sva
