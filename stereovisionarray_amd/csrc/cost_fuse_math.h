// cost_fuse_math.h -- the integer arithmetic of the multi-baseline cost fusion
// (DESIGN.md §2.2c), shared by cost_fuse.hip and a host test program
// (tests/test_multibaseline_cpu.py compiles this header with a C++ compiler and
// checks both functions exhaustively).  Plain C++: no HIP header is needed on
// the host side.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SVA_MB_HD __host__ __device__ inline
#else
#define SVA_MB_HD inline
#endif

namespace sva {
namespace mb {

// The mean of the visible pairs, rounded half up: C_f = (2 * sum + n) / (2 * n)
// for n in 1..32 pairs and sum <= 255 * n.  The division is a multiplication
// by magic(n) = ceil(2^22 / (2n)) and a shift: with x = 2 * sum + n <= 511 * n
// and e = magic * 2n - 2^22 < 2n, x * e < 1022 * n^2 <= 2^20 < 2^22, so
// (x * magic) >> 22 == x / (2n) exactly; x * magic < 256 * 2^22 + 2^20 fits 32
// bits and both factors fit 24 (the device multiplies with v_mul_u32_u24).
constexpr int kMeanShift = 22;

// n in 1..32; 0 for n = 0 (no visible pair: the caller writes 62).
SVA_MB_HD unsigned mean_magic(int n) {
    return n > 0 ? ((1u << kMeanShift) + 2u * (unsigned)n - 1u) / (2u * (unsigned)n) : 0u;
}

// x = 2 * sum + n, magic = mean_magic(n).  (The masks change no value; they
// let the device compiler pick the 24-bit multiply.)
SVA_MB_HD unsigned mean_round(unsigned x, unsigned magic) {
    return ((x & 0xffffffu) * (magic & 0xffffffu)) >> kMeanShift;
}

// How many match distances s = 0, 1, .. keep one axis of the §2.2 offset within
// r >= 0 pixels of room.  The major axis (and both axes of a diagonal step)
// moves s pixels; the minor axis moves (2*s*m + M) / (2*M), which stays <= r
// exactly while s <= (2*M*r + M - 1) / (2*m).  The offset never exceeds s and
// s <= 65535 (dmin + D fits the u16 map), so room beyond 65535 is no limit;
// clamping r there keeps 2*M*r in 32 bits (M <= 255).
SVA_MB_HD int axis_limit(int r, int M, int m, bool major) {
    if (major || m == M) return r + 1;
    const unsigned rc = r < 65535 ? (unsigned)r : 65535u;
    return (int)((2u * (unsigned)M * rc + (unsigned)M - 1u) / (2u * (unsigned)m)) + 1;
}

// lim(p): the matched pixel p + off(dmin + d) of step (sx, sy) lies inside
// [0,W) x [0,H) exactly for d < lim (the offset moves monotonically outwards),
// clamped to 0..D.  Computed from the geometry alone: a cost byte of 62 is
// also a legal inside value.
SVA_MB_HD int pair_lim(int x, int y, int W, int H, int sx, int sy, int dmin, int D) {
    const int ax = sx < 0 ? -sx : sx, ay = sy < 0 ? -sy : sy;
    const int M = ax > ay ? ax : ay, m = ax > ay ? ay : ax;
    int lim = 65536;
    if (sx != 0) {
        const int l = axis_limit(sx > 0 ? W - 1 - x : x, M, m, ax >= ay);
        lim = l < lim ? l : lim;
    }
    if (sy != 0) {
        const int l = axis_limit(sy > 0 ? H - 1 - y : y, M, m, ay > ax);
        lim = l < lim ? l : lim;
    }
    const int d = lim - dmin;
    return d < 0 ? 0 : (d > D ? D : d);
}

}  // namespace mb
}  // namespace sva
