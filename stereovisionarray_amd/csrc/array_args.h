// array_args.h -- the arguments of one camera-array frame (the sva_array_depth*
// entries) and their validation, shared by multi.cpp and the host
// test programs (tests/test_array_args_cpu.py, test_array_sub_args_cpu.py,
// test_cross_check_cpu.py, test_speckle_cpu.py, test_fill_cpu.py and
// test_wmed_cpu.py and test_rectify_cpu.py compile this header with a C++
// compiler under the sanitizers).  Plain C++: no HIP header.
//
// The post-filter chain (DESIGN.md §7 has its table): between its jobs and its
// depth step a frame passes the jobs' maps through the cross-view check, the
// speckle filter, hole filling and the weighted median, in this order, each
// enabled by its flag below (cross, speckle, fill, wmed) with its argument group.
// With rect the frame starts from raw views: they are rectified on the devices
// before the jobs, and with rect_mask the jobs' maps are masked before the chain.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "cost_mixed_math.h"
#include "cross_check_math.h"
#include "fill_math.h"
#include "rectify_math.h"
#include "speckle_math.h"
#include "sva.h"
#include "sva_native_d.h"
#include "wmedian_math.h"

namespace sva {

// What a job of the frame is: a pair (every pair matched on its own, each
// group's maps fused into depth), or a reference camera's whole group fused at
// the cost level, of equal or of mixed baselines (§2.2d).
// Unknown: a route number sva_array_depth_sub does not know; always refused.
enum class ArrayRoute { Pairs, Groups, GroupsMixed, Unknown };

// sva_array_depth_sub's SVA_ARRAY_* route number as a route.
inline ArrayRoute array_route_of(int route) {
    switch (route) {
        case SVA_ARRAY_PAIRS: return ArrayRoute::Pairs;
        case SVA_ARRAY_GROUPS: return ArrayRoute::Groups;
        case SVA_ARRAY_GROUPS_MIXED: return ArrayRoute::GroupsMixed;
        default: return ArrayRoute::Unknown;
    }
}

struct ArrayArgs {
    const uint8_t* const* images = nullptr;   // n_images host views [H][pitch]
    int n_images = 0, W = 0, H = 0;
    size_t pitch = 0;
    const sva_array_pair* pairs = nullptr;
    const int32_t* group_start = nullptr;     // n_groups + 1 offsets into pairs
    int n_pairs = 0, n_groups = 0;
    double f = 0, pixel_size = 0;
    ArrayRoute route = ArrayRoute::Pairs;
    // conf: the jobs run through the confidence instance with this uniqueness,
    // and `mode` picks the fusion of a group's maps (the group routes: always
    // on, one map per group, SVA_FUSE_MEDIAN)
    bool conf = false;
    int uniqueness = 0, mode = SVA_FUSE_MEDIAN;
    const double* unit_baseline = nullptr;    // per group; GroupsMixed only
    // sub (sva_array_depth_sub): every job also writes its f32
    // sub-pixel map, and depth is fused from those maps
    bool sub = false;
    // host outputs, all but depth nullable: per group, then per job
    double* depth = nullptr;
    uint8_t *n_valid = nullptr, *winner = nullptr;
    uint16_t *maps = nullptr, *cost_min = nullptr, *cost_second = nullptr;
    float* subpix = nullptr;                  // per job; sub only
    // cross: the groups' maps go through sva_cross_check_d
    // into a workspace that the later steps read; group routes only
    bool cross = false;
    const int32_t* view_step = nullptr;       // [n_images][2], unit baselines
    int max_diff = 0, min_agree = 0, max_conflict = 0;
    uint8_t *agree = nullptr, *conflict = nullptr;   // host, per group, nullable
    // speckle: the jobs' maps go through sva_filter_speckles_d
    // in place (check = 1: cross is set too); every route
    bool speckle = false;
    int check = 0;                            // the entry's `check`, as given
    int speckle_max_size = 0, speckle_max_diff = 0;
    uint32_t* comp_size = nullptr;            // host, per job, nullable
    // fill (speckle is set too): the jobs' maps go through
    // sva_fill_holes_d in place
    bool fill = false;
    int fill_max_dist = 0, fill_min_found = 1, fill_mode = 0;
    uint8_t* n_found = nullptr;               // host, per job, nullable
    // wmed (fill is set too): the jobs' maps go through
    // sva_weighted_median_d, guided by each job's reference view (wmed_weights
    // null: unguided), into a workspace that the depth step reads.
    // wmed_select 0: every pixel, fill = 1; 1: only the pixels the fill looked at
    bool wmed = false;
    int wmed_radius = 1, wmed_min_support = 1, wmed_select = 0;
    const uint16_t* wmed_weights = nullptr;   // host, 256 entries, nullable
    uint16_t* support = nullptr;              // host, per job, nullable
    // rect (sva_array_depth_rectified; speckle and fill are set
    // too, wmed iff wmed_radius != 0): images are RAW views; every device runs
    // sva_rectify_d over the views it needs, by rect_views[v], and with rect_mask
    // every job's map goes through sva_mask_maps_d with its reference view's valid
    // plane before the cross-view check
    bool rect = false;
    const sva_rectify_view* rect_views = nullptr;   // host, n_images
    int rect_border = 0, rect_mask = 0;
    uint8_t *views_out = nullptr, *valid_out = nullptr;   // host [n_images][H][W], nullable
};

inline int check_params(const sva_sgm_params& p) {
    if (!padded_D(p.D) || p.dmin < 0 || (p.dir == 0 && p.dir_y == 0))
        return SVA_ERR_INVALID_ARG;
    return SVA_OK;
}

// The ratio num/den (both in 1..kMaxRatio) that baseline / unit equals within
// 1e-9 relative: den ascending, the first hit (so the reduced form).  False if
// none.
inline bool baseline_ratio(double baseline, double unit, int32_t* num, int32_t* den) {
    if (!(unit > 0) || !(baseline > 0)) return false;
    const double r = baseline / unit;
    for (int d = 1; d <= mb::kMaxRatio; d++)
        for (int n = 1; n <= mb::kMaxRatio; n++)
            if (std::fabs(r * d - n) <= 1e-9 * n) {
                *num = n;
                *den = d;
                return true;
            }
    return false;
}

// Checks a frame's arguments, in this order for every route:
// the route's options; the sizes and pointers; the ends of group_start; every
// group's size -- all groups, before any pairs[j] is read through group_start;
// every pair; every group's shared values; the mixed route's ratios.  Returns
// the status and the message of the first rule broken.  ratio (GroupsMixed):
// receives every pair's reduced (num, den).
// With a.cross, after all of the above and in this order: the pair route
// (SVA_ERR_UNSUPPORTED); a subpix plane without sub; null view_step; more than
// 32 groups (SVA_ERR_UNSUPPORTED); two groups with one ref; groups whose
// `invalid` differ; groups whose depth scale differs; a pair whose step
// contradicts view_step; the ranges of cross_check_math.h on the groups'
// view_step (components, then duplicates) and on max_diff, min_agree,
// max_conflict.  (The entry itself refuses a `sub` outside 0 / 1 before it
// builds these arguments: ArrayArgs::sub is a bool.)
inline int check_frame_args(const ArrayArgs& a, std::string& msg, std::vector<int32_t>& ratio) {
    auto fail = [&](int code, const std::string& m) {
        msg = m;
        return code;
    };
    const bool group = a.route != ArrayRoute::Pairs, mixed = a.route == ArrayRoute::GroupsMixed;
    if (a.route == ArrayRoute::Unknown) return fail(SVA_ERR_INVALID_ARG, "unknown route");
    if (a.conf) {
        if (a.mode != SVA_FUSE_MIN_COST && a.mode != SVA_FUSE_MAX_MARGIN &&
            a.mode != SVA_FUSE_MEDIAN)
            return fail(SVA_ERR_INVALID_ARG, "unknown fusion mode");
        if (a.uniqueness < 0 || a.uniqueness > 100)
            return fail(SVA_ERR_INVALID_ARG, "uniqueness must be 0..100");
        if (a.winner && a.mode == SVA_FUSE_MEDIAN)
            return fail(SVA_ERR_INVALID_ARG, "the median has no winner map");
    }
    if (a.sub || a.cross || a.speckle) {
        // the entry takes every route's arguments: those of another route are refused
        if (group && a.mode != SVA_FUSE_MEDIAN)
            return fail(SVA_ERR_INVALID_ARG, "the group routes fuse one map: SVA_FUSE_MEDIAN only");
        if (group && (a.n_valid || a.winner))
            return fail(SVA_ERR_INVALID_ARG, "the group routes have no n_valid or winner map");
        if (!mixed && a.unit_baseline)
            return fail(SVA_ERR_INVALID_ARG, "unit_baseline is for SVA_ARRAY_GROUPS_MIXED only");
    }
    if (mixed && !a.unit_baseline) return fail(SVA_ERR_INVALID_ARG, "null unit_baseline");
    if (!a.images || a.n_images <= 0 || !a.pairs || a.n_pairs <= 0 || !a.group_start ||
        a.n_groups <= 0 || !a.depth || a.W <= 0 || a.H <= 0 || a.pitch < (size_t)a.W)
        return fail(SVA_ERR_INVALID_ARG, "bad array arguments");
    const int32_t* gs = a.group_start;
    if (gs[0] != 0 || gs[a.n_groups] != a.n_pairs)
        return fail(SVA_ERR_INVALID_ARG, "group_start must run from 0 to n_pairs");
    // sizes of 1..32 from 0 to n_pairs: group_start is increasing and inside pairs[]
    for (int g = 0; g < a.n_groups; g++) {
        const long long n = (long long)gs[g + 1] - gs[g];
        if (n <= 0 || n > 32) return fail(SVA_ERR_UNSUPPORTED, "groups of 1..32 pairs");
    }
    for (int j = 0; j < a.n_pairs; j++) {
        const sva_array_pair& q = a.pairs[j];
        if (q.ref < 0 || q.ref >= a.n_images || q.other < 0 || q.other >= a.n_images ||
            !a.images[q.ref] || !a.images[q.other] || check_params(q.params))
            return fail(SVA_ERR_INVALID_ARG, "bad pair " + std::to_string(j));
        if (group && q.params.lr_check)
            return fail(SVA_ERR_UNSUPPORTED, "the multi-baseline route has no L/R check");
    }
    for (int g = 0; g < a.n_groups; g++) {
        const std::string of_group = "the pairs of group " + std::to_string(g);
        const sva_array_pair& p0 = a.pairs[gs[g]];
        for (int j = gs[g] + 1; j < gs[g + 1]; j++) {
            const sva_array_pair& q = a.pairs[j];
            if (!group) {
                // the fusion rejects one `invalid` value per group
                if (q.params.invalid != p0.params.invalid)
                    return fail(SVA_ERR_INVALID_ARG,
                                "params.invalid differs within group " + std::to_string(g));
                continue;
            }
            // one reference view, one disparity range, one depth scale per group
            if (q.ref != p0.ref) return fail(SVA_ERR_INVALID_ARG, of_group + " do not share ref");
            if (q.params.D != p0.params.D || q.params.dmin != p0.params.dmin ||
                q.params.P1 != p0.params.P1 || q.params.P2 != p0.params.P2 ||
                q.params.invalid != p0.params.invalid)
                return fail(SVA_ERR_INVALID_ARG,
                            of_group + " must share D, dmin, P1, P2 and invalid");
            const double big = std::max(std::fabs(q.baseline), std::fabs(p0.baseline));
            if (!mixed && !(std::fabs(q.baseline - p0.baseline) <= 1e-9 * big))
                return fail(SVA_ERR_INVALID_ARG, of_group + " have different major-axis baselines");
        }
    }
    // every pair's baseline as a ratio of its group's unit
    if (mixed) ratio.assign(2 * (size_t)a.n_pairs, 0);
    for (int g = 0; mixed && g < a.n_groups; g++)
        for (int j = gs[g]; j < gs[g + 1]; j++) {
            int32_t* rj = &ratio[2 * (size_t)j];
            if (!baseline_ratio(a.pairs[j].baseline, a.unit_baseline[g], rj, rj + 1))
                return fail(SVA_ERR_INVALID_ARG,
                            "the baseline of pair " + std::to_string(j) +
                                " is no num/den (1..8 each) of its group's unit baseline");
            // t(s) >= s / kMaxRatio - 1: past this s it is too far whatever the
            // ratio, and up to it mixed_distance's product stays in 32 bits
            const long long s = (long long)a.pairs[j].params.dmin + a.pairs[j].params.D - 1;
            if (s > 65537ll * mb::kMaxRatio || mb::mixed_distance((int)s, rj[0], rj[1]) > 65535)
                return fail(SVA_ERR_INVALID_ARG,
                            "the match distance of pair " + std::to_string(j) + " exceeds 16 bits");
        }
    if (!a.cross) return SVA_OK;
    // ---- the cross-view check ----
    if (!group)
        return fail(SVA_ERR_UNSUPPORTED,
                    "the cross-view check needs a group route: the pair route's maps share one "
                    "reference camera");
    if (!a.sub && a.subpix)
        return fail(SVA_ERR_INVALID_ARG, "subpix needs sub = 1");
    if (!a.view_step) return fail(SVA_ERR_INVALID_ARG, "null view_step");
    if (a.n_groups > cc::kMaxViews)
        return fail(SVA_ERR_UNSUPPORTED, "the cross-view check takes 1..32 groups");
    auto scale_of = [&](int g) { return mixed ? a.unit_baseline[g] : a.pairs[gs[g]].baseline; };
    for (int g = 1; g < a.n_groups; g++) {
        for (int h = 0; h < g; h++)
            if (a.pairs[gs[g]].ref == a.pairs[gs[h]].ref)
                return fail(SVA_ERR_INVALID_ARG, "groups " + std::to_string(h) + " and " +
                                                     std::to_string(g) + " share ref");
    }
    for (int g = 1; g < a.n_groups; g++)
        if (a.pairs[gs[g]].params.invalid != a.pairs[gs[0]].params.invalid)
            return fail(SVA_ERR_INVALID_ARG,
                        "params.invalid of group " + std::to_string(g) + " differs from group 0's");
    for (int g = 1; g < a.n_groups; g++) {
        const double s0 = scale_of(0), sg = scale_of(g);
        if (!(std::fabs(sg - s0) <= 1e-9 * std::max(std::fabs(sg), std::fabs(s0))))
            return fail(SVA_ERR_INVALID_ARG, "the depth scale of group " + std::to_string(g) +
                                                 " differs from group 0's");
    }
    for (int j = 0; j < a.n_pairs; j++) {
        const sva_array_pair& q = a.pairs[j];
        const long long dx = q.params.dir, dy = q.params.dir_y;
        const long long M = std::max(std::llabs(dx), std::llabs(dy));
        const long long num = mixed ? ratio[2 * (size_t)j] : 1;
        const long long den = mixed ? ratio[2 * (size_t)j + 1] : 1;
        const long long ex = (long long)a.view_step[2 * q.other] - a.view_step[2 * q.ref];
        const long long ey = (long long)a.view_step[2 * q.other + 1] - a.view_step[2 * q.ref + 1];
        if (ex * M * den != dx * num || ey * M * den != dy * num)
            return fail(SVA_ERR_INVALID_ARG,
                        "the step of pair " + std::to_string(j) + " contradicts view_step");
    }
    std::vector<int32_t> vs(2 * (size_t)a.n_groups);
    for (int g = 0; g < a.n_groups; g++) {
        vs[2 * (size_t)g] = a.view_step[2 * a.pairs[gs[g]].ref];
        vs[2 * (size_t)g + 1] = a.view_step[2 * a.pairs[gs[g]].ref + 1];
    }
    const char* m = cc::step_range_error(vs.data(), a.n_groups);
    if (!m) m = cc::step_distinct_error(vs.data(), a.n_groups);
    if (!m) m = cc::thresholds_error(a.max_diff, a.min_agree, a.max_conflict);
    if (m) return fail(SVA_ERR_INVALID_ARG, m);
    return SVA_OK;
}

// check_frame_args, and with a.speckle after all of its rules -- those of
// a.cross among them, which the entry sets iff check == 1 -- in this order: a
// check outside 0 / 1; with check = 0, an agree or conflict plane, then a subpix
// plane without sub; speckle_max_size < 0; speckle_max_diff < 0.  With a.fill
// after those: fill_max_dist, fill_min_found, fill_mode out of range.  With
// a.wmed after those: wmed_radius, wmed_min_support out of range, wmed_select
// outside 0 / 1.  With a.rect those three are checked whether a.wmed or not, a
// wmed_radius of 0 allowed (the median off), and after them: a null rect_views;
// the first rule a view breaks (rc::view_error, view 0 first); rect_border
// outside 0..255; rect_mask outside 0 / 1.
inline int check_array_args(const ArrayArgs& a, std::string& msg, std::vector<int32_t>& ratio) {
    if (int st = check_frame_args(a, msg, ratio)) return st;
    if (!a.speckle) return SVA_OK;
    auto fail = [&](const char* m) {
        msg = m;
        return (int)SVA_ERR_INVALID_ARG;
    };
    if (a.check != 0 && a.check != 1) return fail("check must be 0 or 1");
    if (a.check == 0 && (a.agree || a.conflict))
        return fail("agree and conflict need check = 1");
    if (a.check == 0 && !a.sub && a.subpix) return fail("subpix needs sub = 1");
    if (const char* m = sp::thresholds_error(a.speckle_max_size, a.speckle_max_diff))
        return fail(m);
    if (a.fill)
        if (const char* m = fl::thresholds_error(a.fill_max_dist, a.fill_min_found, a.fill_mode))
            return fail(m);
    if (a.wmed || a.rect) {
        const int radius = a.rect && a.wmed_radius == 0 ? 1 : a.wmed_radius;
        if (const char* m = wm::thresholds_error(radius, a.wmed_min_support, 1)) return fail(m);
        if (a.wmed_select != 0 && a.wmed_select != 1) return fail("wmed select must be 0 or 1");
    }
    if (a.rect) {
        if (!a.rect_views) return fail("null rect");
        for (int v = 0; v < a.n_images; v++)
            if (const char* m = rc::view_error(a.rect_views[v])) {
                msg = std::string(m) + " (view " + std::to_string(v) + ")";
                return (int)SVA_ERR_INVALID_ARG;
            }
        if (a.rect_border < 0 || a.rect_border > 255) return fail("border must be 0..255");
        if (a.rect_mask != 0 && a.rect_mask != 1) return fail("mask must be 0 or 1");
    }
    return SVA_OK;
}

// Which views does each device need?  Pair j runs on device dev_of[j] and needs
// its ref and its other there.  With refs_on_0 (the weighted median stage: the
// guide of a job is its reference view, and the filter runs on device 0; the
// rectified frame's mask: the valid plane of a job's reference view is made where
// the view is rectified, and sva_mask_maps_d runs on device 0) the reference view
// of every pair is needed on device 0 as well.  Out: slot_of[d][v],
// the slot of view v in device d's image buffer (-1: not needed there), slots
// numbered in the order the pairs name them, the extra references of device 0
// last; n_need[d], the number of slots; used[v], whether any device needs v.
inline void plan_views(int n_devices, int n_images, const sva_array_pair* pairs, int n_pairs,
                       const int32_t* dev_of, bool refs_on_0,
                       std::vector<std::vector<int>>& slot_of, std::vector<int>& n_need,
                       std::vector<char>& used) {
    slot_of.assign(n_devices, std::vector<int>(n_images, -1));
    n_need.assign(n_devices, 0);
    used.assign(n_images, 0);
    auto need = [&](int d, int v) {
        used[v] = 1;
        int& s = slot_of[d][v];
        if (s < 0) s = n_need[d]++;
    };
    for (int j = 0; j < n_pairs; j++) {
        need(dev_of[j], pairs[j].ref);
        need(dev_of[j], pairs[j].other);
    }
    for (int j = 0; refs_on_0 && j < n_pairs; j++) need(0, pairs[j].ref);
}

}  // namespace sva
