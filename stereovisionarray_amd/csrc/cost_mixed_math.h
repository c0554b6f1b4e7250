// cost_mixed_math.h -- the integer arithmetic of mixed-baseline Mode S
// (DESIGN.md §2.2d), shared by cost_mixed.hip, cost_fuse.hip, the host route
// and a host test program (tests/test_mixed_cpu.py compiles this header with a
// C++ compiler and checks both functions against brute force).  Plain C++.
#pragma once

#include "cost_fuse_math.h"

namespace sva {
namespace mb {

constexpr int kMaxRatio = 8;   // num and den of a pair's baseline ratio: 1..8

// The match distance of a pair whose major-axis baseline is num/den of the
// group's unit baseline, at group disparity s: s * num / den rounded half up.
// s <= 65535 and num <= 8 keep 2*s*num + den in 32 bits.
SVA_MB_HD int mixed_distance(int s, int num, int den) {
    return (2 * s * num + den) / (2 * den);
}

// lim(p) of such a pair: its matched pixel p + off(t(dmin + d)) lies inside
// [0,W) x [0,H) exactly for d < lim, clamped to 0..D.  limT = the number of
// match distances t = 0, 1, .. that stay inside (pair_lim over the whole u16
// range); t(s) is non-decreasing, and t(s) <= limT - 1 <=> 2*s*num + den <
// 2*den*limT <=> s < ceil((2*den*limT - den) / (2*num)).  limT <= 65536 and
// den <= 8 keep the product in 32 bits.  num = den = 1 gives pair_lim.
SVA_MB_HD int mixed_lim(int x, int y, int W, int H, int sx, int sy, int num, int den, int dmin,
                        int D) {
    const int limT = pair_lim(x, y, W, H, sx, sy, 0, 65536);
    const int slim = limT <= 0 ? 0 : (2 * den * limT - den + 2 * num - 1) / (2 * num);
    const int d = slim - dmin;
    return d < 0 ? 0 : (d > D ? D : d);
}

}  // namespace mb
}  // namespace sva
