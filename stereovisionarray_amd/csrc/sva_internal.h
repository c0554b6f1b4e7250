// sva_internal.h -- context, workspace and kernel-launcher declarations shared
// by the C-ABI (sva_api.cpp) and the HIP kernel translation units.
#pragma once

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "agg_plan.h"
#include "sva.h"
#include "sva_native_d.h"
#include "sva_tuning.h"

namespace sva {

// Per-kernel hipEvent timing on the context stream.  Events are only recorded
// while timing is enabled; resolution happens lazily in kernel_time().
struct KernelTimer {
    bool enabled = false;
    int mode = 0;              // SVA_TIMING_ALL / _PATHS / _AGG (sva_set_timing)
    struct Pending {
        std::string name;
        hipEvent_t start, stop;
    };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;
    std::map<std::string, std::pair<double, int64_t>> totals;  // ms, count

    hipEvent_t get_event();
    void begin(hipStream_t s, const char* name, hipEvent_t* start_out);
    void end(hipStream_t s, const char* name, hipEvent_t start);
    hipError_t resolve();  // fold pending into totals (synchronises on each stop event)
    void release_all();
};

// Device workspace grown on demand (never shrinks within a context).
struct DevBuf {
    void* ptr = nullptr;
    size_t bytes = 0;
    unsigned flags = 0;   // hipExtMallocWithFlags flags (0 = hipMalloc)
    hipError_t ensure(size_t n);
    void release();
};

struct Ctx {
    int device = -1;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string last_error;
    KernelTimer timer;
    // Mode S workspace
    DevBuf census_l, census_r, cost, paths, ckpt, scratch_u16, disp_r;
    // host-pointer staging
    DevBuf in_a, in_b, in_mask, out_a, out_b, out_c;
    // refinement / 3-D workspace (refine.hip)
    DevBuf in_c, shifted, keys, counts, total;
    // the box-sum refinement route's tables (refine.hip sat_plan; sva.h gives the size)
    DevBuf refine_ws;
    // SVA_DEBUG_REFINE_ROUTE (0 = automatic, 1 = box-sum route for every k >= 1)
    // and SVA_DEBUG_REFINE_LAST_ROUTE (0 = refine_box_kernel, 1 =
    // refine_kernel<ND>, 2 = box-sum route, -1 = no refine launch yet)
    int dbg_refine_route = 0;
    int last_refine_route = -1;
    // SVA_DEBUG_CROSS_ORDER: cross_check's block order (-1 = tune::kCrossTileMajor,
    // 0 = view-major, 1 = tile-major)
    int dbg_cross_order = -1;
    // the speckle filter's label and count planes (speckle.hip; sva.h gives the size)
    DevBuf speckle_ws;
    // hole filling's key planes (fill.hip; sva.h gives the size), and
    // SVA_DEBUG_FILL_SEGMENT: the scan's segment length (0 = tune::kFillSegment)
    DevBuf fill_ws;
    // the host entry of the weighted median filter packs its guides here
    DevBuf wmed_guides;
    int dbg_fill_segment = 0;
    // Mode R's split plane loop: one first-minimum key per pixel (refpath.hip).
    // ref_finalize_kernel puts every key it reads back to all-ones, so after
    // the first call only a grown buffer needs the memset: ref_keys_clean =
    // leading bytes known to be all-ones (of allocation ref_keys_alloc)
    DevBuf ref_keys;
    size_t ref_keys_clean = 0;
    const void* ref_keys_alloc = nullptr;
    int cu_count = 256;
    // sva_batch_sgm's per-context pipeline (copy streams, events, pinned and
    // device staging), created on first use and kept for later calls
    std::shared_ptr<void> batch_lane;
    // sva_disparity_sgm_batch_d: side streams for the frames' census + cost
    // (fork / join through events on `stream`), their census workspaces
    std::vector<hipStream_t> side;
    std::vector<hipEvent_t> side_done;
    hipEvent_t fork = nullptr;
    DevBuf census_side;
    // sva_set_debug switches (include/sva.h SVA_DEBUG_*): Mode R shares per
    // tile forced (0 = automatic), and the batch route's injected cost-launch
    // failure (1-based frame of the next call, 0 = off)
    int dbg_plane_split = 0;
    int dbg_fail_cost_at = 0;
    // SVA_DEBUG_DIAG_ROUTE: the diagonal route of the last frame's aggregation
    // (0 = four volumes, 1 = pair volumes)
    int last_diag_route = 0;
    // SVA_DEBUG_DIAG_PAIR_MIN_PIXELS: smallest W * H on the pair route
    // (-1 = tune::kDiagPairMinPixels)
    int64_t dbg_pair_min_pixels = -1;
    // sva_reserve's placement check: sets to time (0 = tune::kPlacementTrials),
    // and the kept / slowest set's path-kernel time of the last check (ns)
    int placement_trials = 0;
    int64_t placement_ns = 0, placement_worst_ns = 0;
    const void* placement_paths = nullptr;   // the path buffer the last check chose
};

// Which launches a timing mode records: SVA_TIMING_ALL every one,
// SVA_TIMING_PATHS only the path-aggregation launch "sgm_paths" (the
// roofline-graded kernel), SVA_TIMING_AGG that one and the kernel that
// finishes the aggregation, "wta_hv" (bench.py's aggregation roofline).
inline bool timer_wants(const KernelTimer& t, const char* name) {
    if (!t.enabled) return false;
    if (t.mode == SVA_TIMING_ALL) return true;
    if (std::strcmp(name, "sgm_paths") == 0) return true;
    return t.mode == SVA_TIMING_AGG && std::strcmp(name, "wta_hv") == 0;
}

// RAII helper: records timing events around one launch when enabled.
struct ScopedKernelTimer {
    Ctx& c;
    const char* name;
    hipEvent_t start = nullptr;
    ScopedKernelTimer(Ctx& ctx, const char* n) : c(ctx), name(n) {
        if (timer_wants(c.timer, name)) c.timer.begin(c.stream, name, &start);
    }
    ~ScopedKernelTimer() {
        if (c.timer.enabled && start) c.timer.end(c.stream, name, start);
    }
};

// Timing of one launch through hipExtLaunchKernelGGL's start/stop events: the
// runtime stamps them from the kernel's own dispatch, so no separate event
// packets enter the stream (used for the two aggregation kernels, the ones
// bench.py times inside its timed region).  start/stop stay null when timing
// is off.
struct DispatchTimer {
    Ctx& c;
    const char* name;
    hipEvent_t start = nullptr, stop = nullptr;
    bool used = false;   // set by the launch that received start/stop
    DispatchTimer(Ctx& ctx, const char* n) : c(ctx), name(n) {
        if (timer_wants(c.timer, name)) {
            start = c.timer.get_event();
            stop = start ? c.timer.get_event() : nullptr;
            if (!stop && start) { c.timer.pool.push_back(start); start = nullptr; }
        }
    }
    ~DispatchTimer() {
        if (start && stop && used)
            c.timer.pending.push_back(KernelTimer::Pending{name, start, stop});
        else if (start && stop) {
            c.timer.pool.push_back(start);
            c.timer.pool.push_back(stop);
        }
    }
};

// ------------------------------------------------------------- launchers --
// All launchers enqueue on ctx.stream and return the launch status.

// census.hip
hipError_t launch_census(Ctx& c, const uint8_t* img, int W, int H, size_t pitch, uint64_t* out);
hipError_t launch_census_pair(Ctx& c, const uint8_t* left, const uint8_t* right, int W, int H,
                              size_t pitch, uint64_t* out_l, uint64_t* out_r);
// cost.hip
// Census + cost in one kernel (census_cost.hip), 1-D steps (dir = +-1).
bool census_cost_supported(int D);
// D is the native volume width (64/128/192/256); dreal <= D the caller's
// disparity count: d >= dreal gets cost 255 (0 = D).
hipError_t launch_census_cost(Ctx& c, const uint8_t* left, const uint8_t* right, int W, int H,
                              size_t pitch, int D, int dmin, int dir, uint8_t* C, int dreal = 0);
// Census + cost in one kernel for 2-D steps (census_cost2.hip): steps whose
// primitive form has |by| = 1 and |bx| <= 3, native D.
bool census_cost2_supported(int D, int sx, int sy);
hipError_t launch_census_cost2(Ctx& c, const uint8_t* left, const uint8_t* right, int W, int H,
                               size_t pitch, int D, int dmin, int sx, int sy, uint8_t* C,
                               int dreal = 0);
hipError_t launch_cost(Ctx& c, const uint64_t* cl, const uint64_t* cr, int W, int H, int D,
                       int dmin, int dir, uint8_t* C, int dreal = 0);
// sgm_paths.hip and wta_hv.hip -- the aggregation, described by an AggPlan
// (agg_plan.h: route, sizes, plane offsets and the legality rules; layout table
// in DESIGN.md §4.9a).  launch_paths runs all 8 directions in one launch: eight
// volumes, or the tile pipeline's diagonal volumes plus checkpoints (and minima
// planes), from which launch_wta_hv recomputes the other four directions per
// tile, sums and picks d* into disp / sub (W*H each per frame).  A plan that is
// not plan_valid, or buffers that do not fit it, are hipErrorInvalidValue.
hipError_t launch_paths(Ctx& c, const AggPlan& p, const AggBuffers& b);
bool paths_supported(int D);   // is_native_d
// The WTA's confidence outputs, a kernel argument of the
// confidence instances: W*H u16 planes (each nullable; a batch launch: one per
// frame back to back, like disp), the uniqueness percentage 0..100 (0 = no
// filter) and the disparity a rejected pixel gets, both one value per launch.
struct ConfOut {
    uint16_t* cost_min = nullptr;
    uint16_t* cost_second = nullptr;
    int uniqueness = 0;
    unsigned invalid = 0xffffu;
};
// cf set: the confidence instance of the same kernel.
hipError_t launch_wta_hv(Ctx& c, const AggPlan& p, const AggBuffers& b, uint16_t* disp, float* sub,
                         const ConfOut* cf = nullptr);
// wta.hip
hipError_t launch_sum(Ctx& c, const uint8_t* L8, int W, int H, int D, uint16_t* S);
hipError_t launch_wta_from_sum(Ctx& c, const uint16_t* S, int W, int H, int D, int dmin,
                               uint16_t* disp, float* sub, const ConfOut* cf = nullptr);
hipError_t launch_lr_check(Ctx& c, uint16_t* disp_l, const uint16_t* disp_r, float* sub, int W, int H,
                           int sx, int sy, int max_diff, uint16_t invalid);
// 2-D matching step (sy != 0); sy == 0 forwards to launch_cost(dir = sx).
hipError_t launch_cost2(Ctx& c, const uint64_t* cl, const uint64_t* cr, int W, int H, int D,
                        int dmin, int sx, int sy, uint8_t* C, int dreal = 0);
// cost_fuse.hip -- multi-baseline cost fusion: n <= 32 cost
// volumes [H][W][D] (native D), volume i at volumes + i * stride, of one
// reference image matched along steps[i] = (sx, sy), into `fused`: per cell the
// mean (rounded half up) over the pairs whose matched pixel is inside the
// image, 62 where none is, 255 at d >= dreal (0 = D).  ratios null: equal
// baselines.  Else the mixed-baseline instance: pair i's
// major-axis baseline is ratios[2i] / ratios[2i+1] of the group's unit baseline
// (each in 1..8), and it is visible where its matched pixel at distance
// t(dmin + d) is inside.
hipError_t launch_cost_fuse(Ctx& c, const uint8_t* volumes, size_t stride, int n, int W, int H,
                            int D, int dreal, int dmin, const int32_t* steps,
                            const int32_t* ratios, uint8_t* fused);
// cost_mixed.hip -- the cost volume of one such pair from two census maps
// (DESIGN.md §2.2d, §4.20): C(p, d) against the matched pixel at distance
// t(dmin + d) = (dmin + d) * num / den rounded half up along (sx, sy).  Native
// D; num, den in 1..8; 255 at d >= dreal (0 = D).
hipError_t launch_cost_mixed(Ctx& c, const uint64_t* cen_ref, const uint64_t* cen_oth, int W, int H,
                             int D, int dmin, int sx, int sy, int num, int den, uint8_t* C,
                             int dreal = 0);
// fuse.hip -- depth fusion over n_maps <= 32 u16 maps [n_maps][np] (DESIGN.md
// §2.6, §2.6b, §2.6c).  num[i] = baseline_i * f (host-computed, the oracle's f64
// product).  mode SVA_FUSE_MEDIAN: the median of the valid maps' depths (cost
// planes and winner unused).  SVA_FUSE_MIN_COST / SVA_FUSE_MAX_MARGIN: the depth
// of the valid map with the smallest cost_min / the largest cost_second -
// cost_min (cost_second nullable for MIN_COST); winner (nullable) gets its
// index, 0xFF if none.  subpix (nullable, f32 [n_maps][np]): the depths come
// from it, and a map is valid where its u16 disparity is and subpix > 0.
hipError_t launch_fuse(Ctx& c, const uint16_t* disps, const float* subpix, const uint16_t* cost_min,
                       const uint16_t* cost_second, int n_maps, size_t np, const double* num,
                       double pixel_size, uint16_t invalid, int mode, double* depth,
                       uint8_t* n_valid, uint8_t* winner);
// cross_check.hip -- the cross-view consistency check: n <= 32
// maps [n][H][W] of one unit baseline, view_step [n][2] (host); subpix / out_sub
// (f32), agree, conflict (u8) nullable, out_sub needs subpix; W * H < 2^31.
// tile_major: the block order (tune::kCrossTileMajor), speed only.
hipError_t launch_cross_check(Ctx& c, const uint16_t* disps, const float* subpix, int n, int W,
                              int H, const int32_t* view_step, uint16_t invalid, int max_diff,
                              int min_agree, int max_conflict, int tile_major, uint16_t* out,
                              float* out_sub, uint8_t* agree, uint8_t* conflict);
// speckle.hip -- the speckle filter: n maps [n][H][W], W * H <
// 2^31; label, count: u32 workspace planes [n][H][W] (both null: max_size = 0
// and no comp_size, a copy); subpix / out_sub (f32) and comp_size (u32)
// nullable, out_sub needs subpix; out may be disps and out_sub subpix.
hipError_t launch_speckle(Ctx& c, const uint16_t* disps, const float* subpix, int n, int W, int H,
                          uint16_t invalid, int max_size, int max_diff, uint32_t* label,
                          uint32_t* count, uint16_t* out, float* out_sub, uint32_t* comp_size);
// fill.hip -- hole filling: n maps [n][H][W], W * H < 2^31;
// keys: u32 workspace planes [n][8][H][W], null iff max_dist = 0 (a copy);
// segment >= 1: the scan's segment length; subpix / out_sub (f32) and n_found
// (u8) nullable, out_sub needs subpix; out may be disps and out_sub subpix.
hipError_t launch_fill(Ctx& c, const uint16_t* disps, const float* subpix, int n, int W, int H,
                       uint16_t invalid, int max_dist, int min_found, int mode, int segment,
                       uint32_t* keys, uint16_t* out, float* out_sub, uint8_t* n_found);
// wmedian.hip -- the weighted median filter: n maps [n][H][W],
// W * H < 2^31; guides: a HOST array of n device images, `guide_pitch` >= W bytes a
// row, and weights a HOST array of 256, both null for the unguided filter, both
// read before the call returns; select (u8), subpix / out_sub (f32) and support
// (u16) nullable, out_sub needs subpix; no output may overlap an input.
hipError_t launch_wmedian(Ctx& c, const uint16_t* disps, const float* subpix,
                          const uint8_t* const* guides, size_t guide_pitch, const uint16_t* weights,
                          const uint8_t* select, int n, int W, int H, uint16_t invalid, int radius,
                          int min_support, int fill, uint16_t* out, float* out_sub,
                          uint16_t* support);
// rectify.hip -- rectification: n views [n][sh][src_pitch] onto
// [n][H][out_pitch]; views a HOST array of n, read before the call returns; valid
// (u8, out's layout) and map (i32 [n][H][W][2]) nullable.  Sizes 1..32767.
hipError_t launch_rectify(Ctx& c, const uint8_t* src, int n, int sw, int sh, size_t src_pitch,
                          const sva_rectify_view* views, int W, int H, size_t out_pitch,
                          int border, uint8_t* out, uint8_t* valid, int32_t* map);
// sva_mask_maps (§2.5g): out = valid ? disps : invalid, out_sub = valid ? subpix : NaN.
hipError_t launch_mask_maps(Ctx& c, const uint16_t* disps, const float* subpix,
                            const uint8_t* valid, int n, int W, int H, uint16_t invalid,
                            uint16_t* out, float* out_sub);
// refpath.hip
hipError_t launch_ref_endpoints(Ctx& c, int W, int H, const sva_camera& cref,
                                const sva_camera& coth, int k, double t_near, double t_far,
                                int32_t* ends, uint8_t* valid);
hipError_t launch_ref_match(Ctx& c, const uint8_t* ref, const uint8_t* other, int W, int H,
                            size_t pitch, const uint8_t* mask, const int32_t* ends,
                            const uint8_t* valid_in, int k, uint8_t* disp_u8,
                            uint16_t* disp_u16, uint8_t* valid_out);
// refine.hip
hipError_t launch_shift_perspective(Ctx& c, const sva_camera& in, const sva_camera& out,
                                    const uint8_t* disp, const uint8_t* img, int W, int H,
                                    size_t pitch, uint8_t* shifted, bool zero_fill = false);
hipError_t launch_refine(Ctx& c, const uint8_t* disp, const uint8_t* center,
                         const uint8_t* shifted, const uint8_t* mask, int W, int H, size_t pitch,
                         int k, const sva_camera& c0, const sva_camera& c1, uint8_t* out,
                         int* fault);
hipError_t launch_shift_perspective2(Ctx& c, const sva_camera& in, const sva_camera& out,
                                     const double* depth, int W, int H, unsigned* keys,
                                     double* shifted);
hipError_t launch_points_to_depth(Ctx& c, const double* pts, long long n, const sva_camera& cam,
                                  int W, int H, unsigned* keys, double* depth);
size_t d2p_units(int W, int H);
hipError_t launch_depth_to_points(Ctx& c, const double* depth, int W, int H,
                                  const sva_camera& cam, unsigned* counts, long long* total,
                                  double* pts);
// ingest.hip
void resize_half_size(int W, int H, int* dw, int* dh);
// evaluation (evaluate.hip): resize(src, dst, Size(dw, dh)) INTER_LINEAR on
// dense f64; with ref non-null dst = resized * scale + ref * -scale + 0.
hipError_t launch_resize_linear(Ctx& c, const double* src, int sw, int sh, double* dst, int dw,
                                int dh, const double* ref, double scale);
size_t masked_mean_workspace();
hipError_t launch_masked_mean(Ctx& c, const double* img, const uint8_t* mask, size_t n,
                              void* ws, double* mean);
hipError_t launch_resize_half(Ctx& c, const uint8_t* src, int W, int H, size_t pitch,
                              uint8_t* dst, size_t dpitch);
hipError_t launch_disp_to_depth(Ctx& c, const uint8_t* disp, int n, double cam_distance,
                                double f, double pixel_size, double* depth);

}  // namespace sva
