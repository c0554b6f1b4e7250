// speckle_math.h -- the speckle filter's rule as plain C++
// shared by the kernels (speckle.hip), the argument checks (sva_api.cpp,
// array_args.h) and the host test programs (tests/test_speckle_cpu.py).  No HIP
// header.
//
// A pixel is valid iff d != invalid and d != 0 (cc::valid, the rule of fusion
// and of the cross-view check).  Two 4-neighbours of one map are linked iff both
// are valid and |d1 - d2| <= max_diff -- against the neighbour, never against a
// seed.  A valid pixel whose component has at most max_size pixels is removed.
// d <= 65535, so the difference lies in -65535..65535 and a max_diff above
// 65535 changes nothing: it is clamped there.
#pragma once

#include <cstdint>

#include "cross_check_math.h"

namespace sva {
namespace sp {

constexpr int kMaxDiff = 65535;            // max_diff beyond this changes nothing
constexpr uint32_t kNoLabel = 0xFFFFFFFFu; // the label of a pixel that is not valid

SVA_CC_HD inline int clamp_diff(int max_diff) { return max_diff > kMaxDiff ? kMaxDiff : max_diff; }

// s, t: the values of two 4-neighbours; max_diff in 0..kMaxDiff.
SVA_CC_HD inline bool linked(unsigned s, unsigned t, unsigned invalid, int max_diff) {
    if (!cc::valid(s, invalid) || !cc::valid(t, invalid)) return false;
    const int diff = (int)s - (int)t;
    return diff <= max_diff && -diff <= max_diff;
}

// size: comp_size of the pixel (0 = not valid); max_size in 0..2^31-1.
SVA_CC_HD inline bool removed(uint32_t size, int max_size) {
    return size != 0u && size <= (uint32_t)max_size;
}

// The argument rule sva_filter_speckles* and sva_array_depth_filtered share:
// the message of the first rule broken, or null.
inline const char* thresholds_error(int max_size, int max_diff) {
    if (max_size < 0) return "speckle max_size must be >= 0";
    if (max_diff < 0) return "speckle max_diff must be >= 0";
    return nullptr;
}

}  // namespace sp
}  // namespace sva
