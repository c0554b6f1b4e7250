// cross_check_math.h -- the cross-view consistency rule as
// plain C++ shared by the kernel (cross_check.hip), the argument checks
// (sva_api.cpp, array_args.h) and the host test program
// (tests/test_cross_check_cpu.py).  No HIP header.
//
// View a's pixel p at unit disparity s is seen by view b at q = p + s * e,
// e = view_step[b] - view_step[a], exact on integers.  All arithmetic fits in
// i32: s <= 65535 and |e| <= 2 * kMaxStep = 510 per component, so |s * e| <=
// 33 422 850 < 2^25; the inside test compares that product with -p and W - p
// (both in i32 because 0 <= p < W < 2^31) and forms q only where it is inside;
// t - s lies in -65535..65535 and max_diff is clamped to 65535, where the rule
// no longer changes.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SVA_CC_HD __host__ __device__
#else
#define SVA_CC_HD
#endif

namespace sva {
namespace cc {

constexpr int kMaxViews = 32;     // n views; min_agree / max_conflict 0..31, the count planes u8
constexpr int kMaxStep = 255;     // |view_step| per component
constexpr int kMaxDiff = 65535;   // max_diff beyond this changes nothing

// What view b says about view a's pixel.
enum Class : int {
    kNone = 0,       // q outside the image, or t not valid: b does not count
    kAgree = 1,      // |t - s| <= max_diff
    kConflict = 2,   // t < s - max_diff: b sees through the point (free-space violation)
    kOccluded = 3,   // t > s + max_diff: something nearer hides the point from b
};

SVA_CC_HD inline bool valid(unsigned d, unsigned invalid) { return d != invalid && d != 0u; }

// q = p + s * e along one axis, if it lies in [0, size).  p in [0, size).
SVA_CC_HD inline bool inside_axis(int p, int s, int e, int size, int* q) {
    const int off = s * e;
    if (off < -p || off >= size - p) return false;
    *q = p + off;
    return true;
}

// The matched pixel of (px, py) at disparity s along step (ex, ey).
SVA_CC_HD inline bool inside(int px, int py, int s, int ex, int ey, int W, int H, int* qx,
                             int* qy) {
    return inside_axis(px, s, ex, W, qx) && inside_axis(py, s, ey, H, qy);
}

// s valid, t = view b's value at q (q inside), max_diff in 0..kMaxDiff.
SVA_CC_HD inline int classify(int s, unsigned t, unsigned invalid, int max_diff) {
    if (!valid(t, invalid)) return kNone;
    const int diff = (int)t - s;
    if (diff < -max_diff) return kConflict;
    if (diff > max_diff) return kOccluded;
    return kAgree;
}

SVA_CC_HD inline bool keep(int agree, int conflict, int min_agree, int max_conflict) {
    return agree >= min_agree && conflict <= max_conflict;
}

// ---- the argument rules sva_cross_check* and sva_array_depth_checked share ----
// Each returns the message of the first rule broken, or null.

// step: [n][2]; every component in -kMaxStep..kMaxStep.
inline const char* step_range_error(const int32_t* step, int n) {
    for (int i = 0; i < 2 * n; i++)
        if (step[i] < -kMaxStep || step[i] > kMaxStep)
            return "view_step components must be -255..255";
    return nullptr;
}

// No two views at the same position (e = 0 would compare a map with itself).
inline const char* step_distinct_error(const int32_t* step, int n) {
    for (int i = 0; i < n; i++)
        for (int k = 0; k < i; k++)
            if (step[2 * i] == step[2 * k] && step[2 * i + 1] == step[2 * k + 1])
                return "two views have the same view_step";
    return nullptr;
}

inline const char* thresholds_error(int max_diff, int min_agree, int max_conflict) {
    if (max_diff < 0) return "max_diff must be >= 0";
    if (min_agree < 0 || min_agree > kMaxViews - 1) return "min_agree must be 0..31";
    if (max_conflict < 0 || max_conflict > kMaxViews - 1) return "max_conflict must be 0..31";
    return nullptr;
}

}  // namespace cc
}  // namespace sva
