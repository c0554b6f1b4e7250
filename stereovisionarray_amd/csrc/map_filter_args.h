// map_filter_args.h -- the arguments of the four map filters of the post-filter
// chain (sva_cross_check, sva_filter_speckles,
// sva_fill_holes, sva_weighted_median and their _d twins), of sva_mask_maps
// (§2.5g) and of sva_rectify (§2.5f), and their validation,
// shared by sva_api.cpp and a host test program
// (tests/test_map_filter_args_cpu.py compiles this header with a C++ compiler
// under the sanitizers).  Plain C++: no HIP header.  The rule functions only
// compare pointers and never read through them, except view_step and guides.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

#include "cross_check_math.h"
#include "fill_math.h"
#include "rectify_math.h"
#include "speckle_math.h"
#include "sva.h"
#include "wmedian_math.h"

namespace sva {

// What every filter takes: n maps [n][H][W] u16 with their optional f32 maps, in
// and out, all on the host or all on the device.
struct MapArgs {
    const uint16_t* disps;
    const float* subpix;
    int n, W, H;
    uint16_t invalid;
    uint16_t* out;
    float* out_sub;
};

struct CrossArgs {
    MapArgs m;
    const int32_t* view_step;   // host, [n][2]
    int max_diff, min_agree, max_conflict;
    uint8_t *agree, *conflict;
};

struct SpeckleArgs {
    MapArgs m;
    int max_size, max_diff;
    uint32_t* comp_size;
};

struct FillArgs {
    MapArgs m;
    int max_dist, min_found, mode;
    uint8_t* n_found;
};

struct WmedArgs {
    MapArgs m;
    const uint8_t* const* guides;   // host array of n images
    size_t guide_pitch;
    const uint16_t* weights;        // host, 256 entries
    const uint8_t* select;
    int radius, min_support, fill;
    uint16_t* support;
};

// sva_mask_maps: one valid plane [H][W] u8 per map.
struct MaskArgs {
    MapArgs m;
    const uint8_t* valid;
};

// sva_rectify: n raw views in, n rectified views out, all on the host or all on
// the device; views is always a host array.
struct RectifyArgs {
    const uint8_t* src;
    int n, src_w, src_h;
    size_t src_pitch;
    const sva_rectify_view* views;
    int out_w, out_h;
    size_t out_pitch;
    int border;
    uint8_t *out, *valid;
    int32_t* map;
};

namespace mf {

// a * b + c bytes.  The count saturates at a quarter of the address space (so that
// four times it still fits): a plane that large overlaps everything.  b > 0.
inline size_t sat_bytes(unsigned long long a, size_t b, size_t c = 0) {
    const size_t cap = ~(size_t)0 / 4;
    return a <= (cap - c) / b ? (size_t)a * b + c : cap;
}

// A plane of a call.  Handed to check_filter with its bytes per pixel of the n maps.
struct Plane {
    const void* ptr;
    size_t bytes;
};

inline bool ranges_overlap(const Plane& a, const Plane& b) {
    const uintptr_t x = (uintptr_t)a.ptr, y = (uintptr_t)b.ptr;
    return a.ptr && b.ptr && x < y + b.bytes && y < x + a.bytes;
}

// What tells the four filters' rules apart.
struct Rules {
    const char* what;      // the filter as its messages name it
    int max_n;             // 0: n has no upper bound
    const char* n_rule;
    bool in_place;         // out may be exactly disps, and out_sub exactly subpix
    bool among;            // the outputs are tested against each other too
    const char* overlap;
};

// The rules of a filter, in sva.h's order: the pointers (other_null: one of the
// filter's own is missing), n, the size, W * H < 2^31, the filter's own rules --
// own() returns the message of the first one broken, or null -- "out_sub needs
// subpix", and last the overlap walk: out, out_sub and own_out against disps,
// subpix, own_in and every guide (guide_bytes each), and against each other.
template <class Own>
inline int check_filter(const MapArgs& m, const Rules& r, bool other_null, Own own, Plane own_in,
                        Plane own_out, const uint8_t* const* guides, size_t guide_pitch,
                        std::string& msg) {
    auto fail = [&](int code, const std::string& text) {
        msg = text;
        return code;
    };
    if (!m.disps || other_null || !m.out) return fail(SVA_ERR_INVALID_ARG, "null pointer");
    if (m.n < 1 || (r.max_n && m.n > r.max_n)) return fail(SVA_ERR_INVALID_ARG, r.n_rule);
    if (m.W <= 0 || m.H <= 0) return fail(SVA_ERR_INVALID_ARG, "image size must be positive");
    if ((unsigned long long)m.W * (unsigned long long)m.H >= (1ull << 31))
        return fail(SVA_ERR_UNSUPPORTED, std::string(r.what) + " needs W * H < 2^31");
    if (const char* text = own()) return fail(SVA_ERR_INVALID_ARG, text);
    if (m.out_sub && !m.subpix) return fail(SVA_ERR_INVALID_ARG, "out_sub needs subpix");
    const size_t b8 = sat_bytes((unsigned long long)m.W * m.H, (size_t)m.n);
    const Plane in[3] = {{m.disps, 2 * b8}, {m.subpix, 4 * b8}, {own_in.ptr, own_in.bytes * b8}};
    const Plane out[3] = {{m.out, 2 * b8}, {m.out_sub, 4 * b8}, {own_out.ptr, own_out.bytes * b8}};
    // H rows of W bytes, guide_pitch apart
    const size_t guide_bytes = guides ? sat_bytes((size_t)(m.H - 1), guide_pitch, (size_t)m.W) : 0;
    bool bad = false;
    for (int o = 0; o < 3 && !bad; o++) {
        for (int i = 0; i < 3; i++)
            bad = bad || (!(r.in_place && o == i && o < 2 && out[o].ptr == in[i].ptr) &&
                          ranges_overlap(out[o], in[i]));
        for (int q = o + 1; r.among && q < 3; q++) bad = bad || ranges_overlap(out[o], out[q]);
        for (int i = 0; guides && i < m.n && !bad; i++)
            bad = ranges_overlap(out[o], {guides[i], guide_bytes});
    }
    return bad ? fail(SVA_ERR_INVALID_ARG, r.overlap) : SVA_OK;
}

const char* const kInPlace =
    "an output overlaps an input or another output (in place: out == disps, out_sub == subpix)";

}  // namespace mf

// Each check_x: the rules of sva_x and sva_x_d; returns the status and the message
// of the first rule broken.  The pointers are the caller's (host or device),
// which is where overlap matters.

// The cross-view check tests out and out_sub against disps and subpix only: not
// against each other, and agree and conflict against nothing.
inline int check_cross(const CrossArgs& a, std::string& msg) {
    const mf::Rules r = {"the cross-view check", cc::kMaxViews, "n_views must be 1..32",
                         false, false, "an output overlaps an input"};
    return mf::check_filter(a.m, r, !a.view_step, [&] {
        const char* t = cc::step_range_error(a.view_step, a.m.n);
        if (!t) t = cc::step_distinct_error(a.view_step, a.m.n);
        if (!t) t = cc::thresholds_error(a.max_diff, a.min_agree, a.max_conflict);
        return t;
    }, {}, {}, nullptr, 0, msg);
}

inline int check_speckle(const SpeckleArgs& a, std::string& msg) {
    const mf::Rules r = {"the speckle filter", 0, "n_maps must be >= 1", true, true, mf::kInPlace};
    return mf::check_filter(a.m, r, false,
                            [&] { return sp::thresholds_error(a.max_size, a.max_diff); }, {},
                            {a.comp_size, 4}, nullptr, 0, msg);
}

inline int check_fill(const FillArgs& a, std::string& msg) {
    const mf::Rules r = {"hole filling", 0, "n_maps must be >= 1", true, true, mf::kInPlace};
    return mf::check_filter(a.m, r, false,
                            [&] { return fl::thresholds_error(a.max_dist, a.min_found, a.mode); },
                            {}, {a.n_found, 1}, nullptr, 0, msg);
}

inline int check_wmed(const WmedArgs& a, std::string& msg) {
    const mf::Rules r = {"the weighted median", 0, "n_maps must be >= 1", false, true,
                         "an output overlaps an input or another output (in place is not offered)"};
    return mf::check_filter(a.m, r, false, [&]() -> const char* {
        if (const char* t = wm::thresholds_error(a.radius, a.min_support, a.fill)) return t;
        if ((a.guides == nullptr) != (a.weights == nullptr)) return "guides and weights go together";
        for (int i = 0; a.guides && i < a.m.n; i++)
            if (!a.guides[i]) return "null guide image";
        if (a.guides && a.guide_pitch < (size_t)a.m.W) return "guide pitch < width";
        return nullptr;
    }, {a.select, 1}, {a.support, 2}, a.guides, a.guide_pitch, msg);
}

inline int check_mask(const MaskArgs& a, std::string& msg) {
    const mf::Rules r = {"masking", 0, "n_maps must be >= 1", true, true, mf::kInPlace};
    return mf::check_filter(a.m, r, !a.valid, [] { return (const char*)nullptr; }, {a.valid, 1},
                            {}, nullptr, 0, msg);
}

// The rules of sva_rectify and sva_rectify_d, in sva.h's order.
inline int check_rectify(const RectifyArgs& a, std::string& msg) {
    auto fail = [&](int code, const std::string& text) {
        msg = text;
        return code;
    };
    if (!a.src || !a.views || !a.out) return fail(SVA_ERR_INVALID_ARG, "null pointer");
    if (a.n < 1) return fail(SVA_ERR_INVALID_ARG, "n must be >= 1");
    if (a.src_w <= 0 || a.src_h <= 0 || a.out_w <= 0 || a.out_h <= 0)
        return fail(SVA_ERR_INVALID_ARG, "image size must be positive");
    if (a.src_w > rc::kMaxSize || a.src_h > rc::kMaxSize || a.out_w > rc::kMaxSize ||
        a.out_h > rc::kMaxSize)
        return fail(SVA_ERR_UNSUPPORTED, "rectification takes widths and heights up to 32767");
    if (a.src_pitch < (size_t)a.src_w || a.out_pitch < (size_t)a.out_w)
        return fail(SVA_ERR_INVALID_ARG, "pitch < width");
    if (a.border < 0 || a.border > 255) return fail(SVA_ERR_INVALID_ARG, "border must be 0..255");
    // n * h rows of w bytes, pitch apart
    const size_t rows_out = mf::sat_bytes((unsigned long long)a.n, (size_t)a.out_h);
    const mf::Plane src = {a.src, mf::sat_bytes(mf::sat_bytes((unsigned long long)a.n,
                                                              (size_t)a.src_h) - 1,
                                                a.src_pitch, (size_t)a.src_w)};
    const size_t out_bytes = mf::sat_bytes(rows_out - 1, a.out_pitch, (size_t)a.out_w);
    const mf::Plane out[3] = {{a.out, out_bytes}, {a.valid, out_bytes},
                              {a.map, mf::sat_bytes(rows_out, (size_t)a.out_w * 8)}};
    for (int o = 0; o < 3; o++) {
        bool bad = mf::ranges_overlap(out[o], src);
        for (int q = o + 1; q < 3; q++) bad = bad || mf::ranges_overlap(out[o], out[q]);
        if (bad)
            return fail(SVA_ERR_INVALID_ARG,
                        "an output overlaps the source or another output (in place is not offered)");
    }
    for (int i = 0; i < a.n; i++)
        if (const char* t = rc::view_error(a.views[i]))
            return fail(SVA_ERR_INVALID_ARG, std::string(t) + " (view " + std::to_string(i) + ")");
    return SVA_OK;
}

}  // namespace sva
