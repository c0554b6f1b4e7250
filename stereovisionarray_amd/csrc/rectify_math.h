// rectify_math.h -- the rectification rule as plain C++ shared
// by the kernel (rectify.hip), the argument checks (map_filter_args.h,
// array_args.h) and the host test program (tests/test_rectify_cpu.py).  No HIP
// header.
//
// An output pixel (x, y) of a view takes its value from the raw view at
//   w  = (h6*x + h7*y) + h8
//   u  = ((h0*x + h1*y) + h2) / w          v  = ((h3*x + h4*y) + h5) / w
//   if k1 == k2 == p1 == p2 == k3 == 0:    sx = u, sy = v
//   else:
//     xn = (u - cx) / fx                   yn = (v - cy) / fy
//     xx = xn*xn   yy = yn*yn   xy = xn*yn   r2 = xx + yy
//     rad = 1 + r2*(k1 + r2*(k2 + r2*k3))
//     xd = (xn*rad + (2*p1)*xy) + p2*(r2 + 2*xx)
//     yd = (yn*rad + p1*(r2 + 2*yy)) + (2*p2)*xy
//     sx = xd*fx + cx                      sy = yd*fy + cy
//   inside = w > 0 and -2^20 < sx < 2^20 and -2^20 < sy < 2^20   (false on NaN)
//   qx = (int)rint(sx*32), qy = (int)rint(sy*32)                 (half to even)
//   X = qx >> 5, a = qx & 31, Y = qy >> 5, b = qy & 31           (arithmetic shift)
//   taps (X,Y) (X+1,Y) (X,Y+1) (X+1,Y+1), weights (32-a)(32-b), a(32-b), (32-a)b, ab
//   value = (sum of weight * tap + 512) >> 10
// all of it f64, every operation rounded on its own (no contraction: the pragma
// below under clang, which compiles the device and the library's host side; a
// host compiler without it must not be given a fused multiply-add to use), the
// division IEEE.  A tap of weight 0 is neither read nor judged; a tap of positive
// weight outside [0, sw) x [0, sh) contributes `border`.  valid = inside and every
// tap of positive weight in the source.  Not inside: value = border, valid = 0,
// qx = qy = INT32_MIN.  |qx|, |qy| < 2^25, so X + 1 and the sums fit an int.
#pragma once

#include <cmath>
#include <cstdint>

#include "cross_check_math.h"
#include "sva.h"

#if defined(__clang__)
#define SVA_RC_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SVA_RC_NO_CONTRACT
#endif

namespace sva {
namespace rc {

constexpr int kMaxSize = 32767;         // of a source or an output, either axis
constexpr double kLimit = 1048576.0;    // 2^20: |sx|, |sy| of an inside pixel lie below it
constexpr int kFracBits = 5;            // the 1/32 px grid
constexpr int32_t kOutside = INT32_MIN; // both map entries of a pixel that is not inside

inline bool is_finite(double v) { return v - v == 0.0; }   // false on NaN and +-inf

// The first rule a view breaks, in sva.h's order, or null.
inline const char* view_error(const sva_rectify_view& v) {
    for (int i = 0; i < 9; i++)
        if (!is_finite(v.h[i])) return "rectify view: h has a non-finite entry";
    if (!is_finite(v.cx) || !is_finite(v.cy)) return "rectify view: cx, cy must be finite";
    if (!is_finite(v.fx) || !is_finite(v.fy) || !(v.fx > 0.0) || !(v.fy > 0.0))
        return "rectify view: fx, fy must be finite and > 0";
    if (!is_finite(v.k1) || !is_finite(v.k2) || !is_finite(v.p1) || !is_finite(v.p2) ||
        !is_finite(v.k3))
        return "rectify view: a distortion coefficient is not finite";
    return nullptr;
}

SVA_CC_HD inline bool has_distortion(const sva_rectify_view& v) {
    return !(v.k1 == 0.0 && v.k2 == 0.0 && v.p1 == 0.0 && v.p2 == 0.0 && v.k3 == 0.0);
}

struct Source {
    double sx, sy;
    bool inside;
};

// Where the output pixel (x, y) looks in the raw view.  distort: has_distortion(v).
SVA_CC_HD inline Source source(const sva_rectify_view& v, bool distort, int x, int y) {
    SVA_RC_NO_CONTRACT
    const double xf = (double)x, yf = (double)y;
    const double w = (v.h[6] * xf + v.h[7] * yf) + v.h[8];
    double sx = ((v.h[0] * xf + v.h[1] * yf) + v.h[2]) / w;
    double sy = ((v.h[3] * xf + v.h[4] * yf) + v.h[5]) / w;
    if (distort) {
        const double xn = (sx - v.cx) / v.fx, yn = (sy - v.cy) / v.fy;
        const double xx = xn * xn, yy = yn * yn, xy = xn * yn, r2 = xx + yy;
        const double rad = 1.0 + r2 * (v.k1 + r2 * (v.k2 + r2 * v.k3));
        const double xd = (xn * rad + (2.0 * v.p1) * xy) + v.p2 * (r2 + 2.0 * xx);
        const double yd = (yn * rad + v.p1 * (r2 + 2.0 * yy)) + (2.0 * v.p2) * xy;
        sx = xd * v.fx + v.cx;
        sy = yd * v.fy + v.cy;
    }
    const bool inside = w > 0.0 && sx > -kLimit && sx < kLimit && sy > -kLimit && sy < kLimit;
    return {sx, sy, inside};
}

struct Sample {
    int32_t qx, qy;   // the source position in 1/32 px, kOutside where not inside
    unsigned value;
    unsigned valid;   // 0 / 1
};

// One output pixel.  tap(X, Y) reads the source at a position inside it; it is
// called for taps of positive weight inside [0, sw) x [0, sh) only.
template <class Tap>
SVA_CC_HD inline Sample sample(const sva_rectify_view& v, bool distort, int x, int y, int sw,
                               int sh, unsigned border, Tap tap) {
    SVA_RC_NO_CONTRACT
    const Source s = source(v, distort, x, y);
    if (!s.inside) return {kOutside, kOutside, border, 0u};
    const int qx = (int)rint(s.sx * 32.0), qy = (int)rint(s.sy * 32.0);
    const int X = qx >> kFracBits, Y = qy >> kFracBits;
    const int a = qx & 31, b = qy & 31;
    const int wx[2] = {32 - a, a}, wy[2] = {32 - b, b};
    unsigned sum = 512u, valid = 1u;
    for (int j = 0; j < 2; j++)
        for (int i = 0; i < 2; i++) {
            const unsigned wt = (unsigned)(wx[i] * wy[j]);
            if (wt == 0u) continue;
            const int tx = X + i, ty = Y + j;
            const bool in = tx >= 0 && tx < sw && ty >= 0 && ty < sh;
            sum += wt * (in ? (unsigned)tap(tx, ty) : border);
            valid = in ? valid : 0u;
        }
    return {qx, qy, sum >> 10, valid};
}

// c = a . b, row-major 3x3; every entry ((a_i0*b_0j + a_i1*b_1j) + a_i2*b_2j).
inline void mul3(const double a[9], const double b[9], double c[9]) {
    SVA_RC_NO_CONTRACT
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            c[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}

// inv = k^-1 by the adjugate.  With k = [k0 .. k8] row-major the cofactors are
//   c0 = k4*k8 - k5*k7   c1 = k2*k7 - k1*k8   c2 = k1*k5 - k2*k4
//   c3 = k5*k6 - k3*k8   c4 = k0*k8 - k2*k6   c5 = k2*k3 - k0*k5
//   c6 = k3*k7 - k4*k6   c7 = k1*k6 - k0*k7   c8 = k0*k4 - k1*k3
// det = (k0*c0 + k1*c3) + k2*c6 and inv[i] = c[i] / det.  False where det is 0
// or not finite.
inline bool inv3(const double k[9], double inv[9]) {
    SVA_RC_NO_CONTRACT
    const double c[9] = {k[4] * k[8] - k[5] * k[7], k[2] * k[7] - k[1] * k[8],
                         k[1] * k[5] - k[2] * k[4], k[5] * k[6] - k[3] * k[8],
                         k[0] * k[8] - k[2] * k[6], k[2] * k[3] - k[0] * k[5],
                         k[3] * k[7] - k[4] * k[6], k[1] * k[6] - k[0] * k[7],
                         k[0] * k[4] - k[1] * k[3]};
    const double det = (k[0] * c[0] + k[1] * c[3]) + k[2] * c[6];
    if (!is_finite(det) || det == 0.0) return false;
    for (int i = 0; i < 9; i++) inv[i] = c[i] / det;
    return true;
}

// sva_rectify_view_of: h = K_raw . (R . K_ideal^-1), the inverse by inv3 first,
// then mul3(R, inverse), then mul3(K_raw, that); cx, cy, fx, fy from K_raw, the
// coefficients copied.  The first rule broken, or null: a non-finite input;
// K_raw with skew (K_raw[1], K_raw[3] != 0) or a bottom row other than 0 0 1; a
// singular K_ideal.  *out is written on success only.
inline const char* view_of(const double K_raw[9], const double dist[5], const double R[9],
                           const double K_ideal[9], sva_rectify_view* out) {
    if (!K_raw || !dist || !R || !K_ideal || !out) return "rectify view: null pointer";
    for (int i = 0; i < 9; i++)
        if (!is_finite(K_raw[i]) || !is_finite(R[i]) || !is_finite(K_ideal[i]))
            return "rectify view: non-finite input";
    for (int i = 0; i < 5; i++)
        if (!is_finite(dist[i])) return "rectify view: non-finite input";
    if (K_raw[1] != 0.0 || K_raw[3] != 0.0) return "rectify view: K_raw has skew";
    if (K_raw[6] != 0.0 || K_raw[7] != 0.0 || K_raw[8] != 1.0)
        return "rectify view: K_raw's bottom row must be 0 0 1";
    double inv[9], m[9];
    if (!inv3(K_ideal, inv)) return "rectify view: K_ideal is singular";
    mul3(R, inv, m);
    mul3(K_raw, m, out->h);
    out->cx = K_raw[2];
    out->cy = K_raw[5];
    out->fx = K_raw[0];
    out->fy = K_raw[4];
    out->k1 = dist[0];
    out->k2 = dist[1];
    out->p1 = dist[2];
    out->p2 = dist[3];
    out->k3 = dist[4];
    return nullptr;
}

// What sva_mask_maps writes for one pixel: the u16 value.
SVA_CC_HD inline unsigned masked(unsigned d, unsigned valid, unsigned invalid) {
    return valid != 0u ? d : invalid;
}

}  // namespace rc
}  // namespace sva
