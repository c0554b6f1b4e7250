// sva_api.cpp -- the C-ABI of libsva.so (declared in include/sva.h).
//
// Host C++ only: argument validation, per-context device/stream/workspace
// management, host<->device staging for the host-pointer entry points, the
// hipEvent kernel timer and the multi-context batch driver.  Every compute
// step is one of the HIP kernels in this directory; there is no CPU path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <functional>
#include <thread>
#include <vector>

#include "cost_mixed_math.h"
#include "map_filter_args.h"
#include "sva_internal.h"
#include "sva_tuning.h"

using namespace sva;

// ------------------------------------------------------------ internals --
namespace sva {

hipEvent_t KernelTimer::get_event() {
    if (!pool.empty()) {
        hipEvent_t e = pool.back();
        pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

void KernelTimer::begin(hipStream_t s, const char*, hipEvent_t* start_out) {
    hipEvent_t e = get_event();
    if (e && hipEventRecord(e, s) == hipSuccess) *start_out = e;
    else *start_out = nullptr;
}

void KernelTimer::end(hipStream_t s, const char* name, hipEvent_t start) {
    hipEvent_t e = get_event();
    if (!e) return;
    if (hipEventRecord(e, s) != hipSuccess) { pool.push_back(e); return; }
    pending.push_back(Pending{name, start, e});
}

hipError_t KernelTimer::resolve() {
    hipError_t st = hipSuccess;
    for (auto& p : pending) {
        float ms = 0.f;
        hipError_t e = hipEventSynchronize(p.stop);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, p.start, p.stop);
        if (e != hipSuccess) st = e;
        auto& t = totals[p.name];
        t.first += ms;
        t.second += 1;
        pool.push_back(p.start);
        pool.push_back(p.stop);
    }
    pending.clear();
    return st;
}

void KernelTimer::release_all() {
    for (auto& p : pending) {
        (void)hipEventDestroy(p.start);
        (void)hipEventDestroy(p.stop);
    }
    pending.clear();
    for (auto e : pool) (void)hipEventDestroy(e);
    pool.clear();
}

hipError_t DevBuf::ensure(size_t n) {
    if (n <= bytes && ptr) return hipSuccess;
    if (ptr) {
        (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
    size_t want = std::max<size_t>(n, 256);
    hipError_t e = flags ? hipExtMallocWithFlags(&ptr, want, flags) : hipMalloc(&ptr, want);
    if (e != hipSuccess) {
        ptr = nullptr;
        return e;
    }
    bytes = want;
    return hipSuccess;
}

void DevBuf::release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    bytes = 0;
}

}  // namespace sva

namespace {

Ctx* as_ctx(void* p) { return static_cast<Ctx*>(p); }

int fail(Ctx* c, int code, const std::string& msg) {
    if (c) c->last_error = msg;
    return code;
}

int hip_fail(Ctx* c, hipError_t e, const char* what) {
    std::string m = std::string(what) + ": " + hipGetErrorString(e);
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation)
        return fail(c, SVA_ERR_OUT_OF_MEMORY, m);
    return fail(c, SVA_ERR_DEVICE, m);
}

#define SVA_HIP(c, expr, what)                           \
    do {                                                 \
        hipError_t _e = (expr);                          \
        if (_e != hipSuccess) return hip_fail(c, _e, what); \
    } while (0)

#define SVA_CHECK_CTX(c)                                                       \
    do {                                                                       \
        if (!(c)) return SVA_ERR_INVALID_ARG;                                  \
        if (hipSetDevice((c)->device) != hipSuccess)                           \
            return fail(c, SVA_ERR_DEVICE, "hipSetDevice failed");             \
    } while (0)

int check_image(Ctx* c, const void* a, int W, int H, size_t pitch) {
    if (!a) return fail(c, SVA_ERR_INVALID_ARG, "null image pointer");
    if (W <= 0 || H <= 0) return fail(c, SVA_ERR_INVALID_ARG, "image size must be positive");
    if (pitch < (size_t)W) return fail(c, SVA_ERR_INVALID_ARG, "pitch smaller than width");
    if ((long long)W * H > (1ll << 31) - 1) return fail(c, SVA_ERR_INVALID_ARG, "image too large");
    return SVA_OK;
}

// Shape limits are checked here, before any workspace is allocated: kernels
// launch with gridDim.y = H (lr_check, refine's gathers), which caps H at
// 65535, and every path volume is addressed with 32-bit buffer offsets.
// Whole-frame entry points take any D in 1..256 (run at the padded native
// width); the stage entry points (native = true) read and
// write [..][D] volumes and take D in {64, 128, 192, 256}.
int check_sgm(Ctx* c, const sva_sgm_params* p, int W, int H, bool native = false) {
    if (!p) return fail(c, SVA_ERR_INVALID_ARG, "null params");
    if (p->D <= 0) return fail(c, SVA_ERR_INVALID_ARG, "D must be positive");
    const int Dp = padded_D(p->D);
    if (!Dp) return fail(c, SVA_ERR_UNSUPPORTED, "GPU path built for D in 1..256");
    if (native && !is_native_d(p->D))
        return fail(c, SVA_ERR_UNSUPPORTED,
                    "stage entry points take D in {64,128,192,256} (whole frames: any D <= 256)");
    if (p->dir < -255 || p->dir > 255 || p->dir_y < -255 || p->dir_y > 255 ||
        (p->dir == 0 && p->dir_y == 0))
        return fail(c, SVA_ERR_INVALID_ARG, "(dir, dir_y) must be a nonzero step, |comp| <= 255");
    if (p->dmin < 0) return fail(c, SVA_ERR_INVALID_ARG, "dmin must be >= 0");
    if (p->dmin + p->D > 65535)
        return fail(c, SVA_ERR_INVALID_ARG, "dmin + D must fit the u16 disparity map");
    if (p->P1 < 0 || p->P2 < 0 || p->P1 > 193 || p->P2 > 193)
        return fail(c, SVA_ERR_INVALID_ARG, "penalties must satisfy 0 <= P1, P2 <= 193");
    if (p->lr_check && p->lr_max_diff < 0)
        return fail(c, SVA_ERR_INVALID_ARG, "lr_max_diff must be >= 0");
    if (H > 65535) return fail(c, SVA_ERR_UNSUPPORTED, "H must be <= 65535");
    if (W > 0 && H > 0 && (unsigned long long)W * (unsigned long long)H * (unsigned)Dp >=
                              (1ull << 32))
        return fail(c, SVA_ERR_UNSUPPORTED, "W*H*D must be < 2^32 (32-bit volume offsets)");
    return SVA_OK;
}

// Paths + WTA of the frame pipeline, the tile pipeline: the
// path kernel writes the four diagonal volumes plus horizontal and vertical
// checkpoints, and wta_hv recomputes the other four directions per tile and
// picks d*.  Dp is the native volume width, p->D <= Dp the caller's
// disparities (§4.7).  (The round-2 route of §4.6 -- six volumes, finished
// by wta_h -- was slower at every frame size measured and left in ABI v5.)
// The aggregation's shape for the plans of agg_plan.h.
AggShape agg_shape(int W, int H, int Dp, const sva_sgm_params* p) {
    return AggShape{W, H, Dp, p->D, p->P1, p->P2, p->dmin};
}

// A frame's aggregation, for the product (paths_wta) and for the stage
// entries that run the same plan on a caller's buffers (sva_paths_frame_d,
// sva_wta_frame_d, sva_frame_layout_of).  The route, the sizes and the layout
// are frame_plan's (agg_plan.h); the pixel threshold of the pair route is the
// tuned one unless pair_min_pixels >= 0 (the context's debug override, or the
// layout query's argument).  Its buffers are carve's, over the context's two
// workspaces or the caller's two buffers.
AggPlan frame_agg_plan(long long pair_min_pixels, int W, int H, int Dp, const sva_sgm_params* p) {
    return frame_plan(agg_shape(W, H, Dp, p),
                      pair_min_pixels >= 0 ? pair_min_pixels : tune::kDiagPairMinPixels);
}

// cf set: wta_hv's confidence instance instead of the plain one.
int paths_wta(Ctx* c, const uint8_t* C, int W, int H, const sva_sgm_params* p, int Dp,
              uint16_t* disp, float* sub, const ConfOut* cf = nullptr) {
    if (!is_native_d(Dp)) return fail(c, SVA_ERR_UNSUPPORTED, "no tile pipeline for this D");
    const AggPlan plan = frame_agg_plan(c->dbg_pair_min_pixels, W, H, Dp, p);
    SVA_HIP(c, c->paths.ensure(plan.paths_bytes), "path workspace");
    SVA_HIP(c, c->ckpt.ensure(plan.ckpt_bytes), "checkpoint workspace");
    const AggBuffers b = carve(plan, C, c->paths.ptr, c->ckpt.ptr);
    SVA_HIP(c, launch_paths(*c, plan, b), "paths launch");
    SVA_HIP(c, launch_wta_hv(*c, plan, b, disp, sub, cf), "wta launch");
    c->last_diag_route = plan.route == AggRoute::Pair ? 1 : 0;
    return SVA_OK;
}

// sva_frame_layout of a frame plan.
sva_frame_layout frame_layout(const AggPlan& plan) {
    sva_frame_layout l;
    std::memset(&l, 0, sizeof(l));
    l.route = plan.route == AggRoute::Pair ? 1 : 0;
    l.minima = plan.minima ? 1 : 0;
    l.D = plan.D;
    l.seg = 1 << plan.tg.seg_log2;
    l.nsx = plan.tg.nsx;
    l.nsy = plan.tg.nty;
    l.n_volumes = (int32_t)(plan.paths_bytes / plan.vol);
    l.cost_bytes = plan.vol;
    l.volumes_bytes = plan.paths_bytes;
    l.ckpt_bytes = plan.ckpt_bytes;
    l.hck_off = plan.hck_off;
    l.hck_bytes = plan.tg.hck_bytes;
    l.vck_off = plan.vck_off;
    l.vck_bytes = plan.tg.vck_bytes;
    l.pair_off = plan.pair_off;
    l.pair_bytes = plan.mn_off - plan.pair_off;
    l.hmn_off = plan.mn_off;
    l.hmn_bytes = plan.minima ? plan.tg.hmn_bytes : 0;
    l.vmn_off = plan.mn_off + l.hmn_bytes;
    l.vmn_bytes = plan.minima ? plan.tg.vmn_bytes : 0;
    return l;
}

// Caller buffers of the frame stages against the plan, as check_tile_buffers
// below: an argument error before anything reaches the device.
int check_frame_buffers(Ctx* c, const AggPlan& plan, const void* C, size_t C_bytes,
                        const void* volumes, size_t volumes_bytes, const void* ckpt,
                        size_t ckpt_bytes) {
    if (!C || !volumes || !ckpt) return fail(c, SVA_ERR_INVALID_ARG, "null stage buffer");
    if (C_bytes < plan.vol) return fail(c, SVA_ERR_INVALID_ARG, "cost buffer smaller than [H][W][D]");
    if (volumes_bytes < plan.paths_bytes)
        return fail(c, SVA_ERR_INVALID_ARG, "volume buffer smaller than the layout's volumes_bytes");
    if (ckpt_bytes < plan.ckpt_bytes)
        return fail(c, SVA_ERR_INVALID_ARG, "checkpoint buffer smaller than the layout's ckpt_bytes");
    return SVA_OK;
}

// Buffer sizes of the tile-pipeline stages (sva_tile_layout).
sva_tile_layout tile_layout(int W, int H, int D) {
    sva_tile_layout l;
    std::memset(&l, 0, sizeof(l));
    const AggPlan plan = stage_plan(AggShape{W, H, D});
    l.seg = 1 << plan.tg.seg_log2;
    l.nsx = plan.tg.nsx;
    l.nsy = plan.tg.nty;
    l.cost_bytes = plan.vol;
    l.diag_volumes = kDiagVolumes;
    l.diag_bytes = plan.paths_bytes;
    l.hckpt_bytes = plan.tg.hck_bytes;
    l.vckpt_bytes = plan.tg.vck_bytes;
    return l;
}

// Caller buffers of the tile stages against the layout: every buffer present
// and at least as large as its plane, so that a sizing slip is an argument
// error before anything reaches the device.
int check_tile_buffers(Ctx* c, int W, int H, int D, const void* C, size_t C_bytes,
                       const void* diag, size_t diag_bytes, const void* hck, size_t hck_bytes,
                       const void* vck, size_t vck_bytes) {
    const sva_tile_layout l = tile_layout(W, H, D);
    if (!C || (!diag && l.diag_bytes) || !hck || !vck)
        return fail(c, SVA_ERR_INVALID_ARG, "null stage buffer");
    if (C_bytes < l.cost_bytes) return fail(c, SVA_ERR_INVALID_ARG, "cost buffer smaller than [H][W][D]");
    if (diag_bytes < l.diag_bytes)
        return fail(c, SVA_ERR_INVALID_ARG, "diagonal volume buffer smaller than [4][H][W][D]");
    if (hck_bytes < l.hckpt_bytes)
        return fail(c, SVA_ERR_INVALID_ARG, "horizontal checkpoint buffer smaller than [2][H][nsx][D]");
    if (vck_bytes < l.vckpt_bytes)
        return fail(c, SVA_ERR_INVALID_ARG, "row checkpoint buffer smaller than [2][nsy][W][D]");
    return SVA_OK;
}

// Which kernels form a frame's cost volume (native width Dp, step (dir, dir_y)):
// census + cost in one kernel for 1-D steps (census_cost.hip) and
// for 2-D steps whose primitive form has |dir_y| = 1 and |dir| <= 3 (every rig
// baseline of getCameraPairs and of BASELINE config 4; census_cost2.hip,
// §4.2b), else census_pair followed by cost2.
enum class CostRoute { Fused1D, Fused2D, Split };
CostRoute cost_route(int Dp, int dir, int dir_y) {
    if (dir_y == 0 && Dp >= tune::kCensusCostMinD && census_cost_supported(Dp))
        return CostRoute::Fused1D;
    return census_cost2_supported(Dp, dir, dir_y) ? CostRoute::Fused2D : CostRoute::Split;
}

// One matching role's cost volume C on c.stream: `ref` matched against `oth`
// along (sx, sy).  The split route reads the census maps cen_ref / cen_oth;
// fill = launch census_pair into them first (*what then names a failing
// launch).  The fused routes keep the maps on chip and take neither.
hipError_t form_cost(Ctx& c, CostRoute route, const uint8_t* ref, const uint8_t* oth, int W, int H,
                     size_t pitch, int Dp, const sva_sgm_params* p, int sx, int sy, uint8_t* C,
                     uint64_t* cen_ref, uint64_t* cen_oth, bool fill,
                     const char** what = nullptr) {
    if (route == CostRoute::Fused1D)
        return launch_census_cost(c, ref, oth, W, H, pitch, Dp, p->dmin, sx, C, p->D);
    if (route == CostRoute::Fused2D)
        return launch_census_cost2(c, ref, oth, W, H, pitch, Dp, p->dmin, sx, sy, C, p->D);
    if (fill) {
        const hipError_t e = launch_census_pair(c, ref, oth, W, H, pitch, cen_ref, cen_oth);
        if (e != hipSuccess) {
            if (what) *what = "census launch";
            return e;
        }
    }
    return launch_cost2(c, cen_ref, cen_oth, W, H, Dp, p->dmin, sx, sy, C, p->D);
}

// Mode S on device buffers: census -> cost -> 8 paths -> WTA (-> L/R check).
// Any D in 1..256 runs at the native width Dp = padded_D(D): the cost kernels
// write 255 at d >= D and the WTA ignores those disparities.
// cf set (sva_disparity_sgm_conf*): the reference pass runs the confidence
// instance, which writes the cost planes and applies the uniqueness filter;
// the right-referenced pass of the L/R check stays the plain instance, and
// lr_check_kernel keeps the pixels the filter already marked invalid.
int run_sgm_device(Ctx* c, const uint8_t* left, const uint8_t* right, int W, int H, size_t pitch,
                   const sva_sgm_params* p, uint16_t* disp, float* sub,
                   const ConfOut* cf = nullptr) {
    const int Dp = padded_D(p->D);
    const size_t np = (size_t)W * H, nv = np * (size_t)Dp;
    int s;
    SVA_HIP(c, c->cost.ensure(nv), "cost workspace");
    uint8_t* C = (uint8_t*)c->cost.ptr;
    uint16_t* dr = nullptr;
    if (p->lr_check) {
        SVA_HIP(c, c->disp_r.ensure(np * 2), "lr workspace");
        dr = (uint16_t*)c->disp_r.ptr;
    }
    const CostRoute route = cost_route(Dp, p->dir, p->dir_y);
    uint64_t *cl = nullptr, *cr = nullptr;
    if (route == CostRoute::Split) {
        SVA_HIP(c, c->census_l.ensure(np * 8), "census workspace");
        SVA_HIP(c, c->census_r.ensure(np * 8), "census workspace");
        cl = (uint64_t*)c->census_l.ptr;
        cr = (uint64_t*)c->census_r.ptr;
    }
    const char* what = "cost launch";
    hipError_t e = form_cost(*c, route, left, right, W, H, pitch, Dp, p, p->dir, p->dir_y, C, cl, cr,
                             true, &what);
    if (e != hipSuccess) return hip_fail(c, e, what);
    if ((s = paths_wta(c, C, W, H, p, Dp, disp, sub, cf))) return s;
    if (p->lr_check) {
        // right image as reference: the images (on the split route their
        // census maps, no second census) swap roles, the step flips
        SVA_HIP(c, form_cost(*c, route, right, left, W, H, pitch, Dp, p, -p->dir, -p->dir_y, C, cr,
                             cl, false),
                "cost launch");
        if ((s = paths_wta(c, C, W, H, p, Dp, dr, nullptr))) return s;
        SVA_HIP(c, launch_lr_check(*c, disp, dr, sub, W, H, p->dir, p->dir_y, p->lr_max_diff,
                                   p->invalid),
                "lr launch");
    }
    return SVA_OK;
}

// cf's planes `off` pixels on: a chunk's or a sub-batch's frames of a batch.
ConfOut conf_at(const ConfOut* cf, size_t off) {
    ConfOut r;
    if (cf) r = *cf;
    if (r.cost_min) r.cost_min += off;
    if (r.cost_second) r.cost_second += off;
    return r;
}

// A batch of frames of one shape through few launches of each aggregation
// kernel: the cost volume of every frame (census + cost per
// frame, each along its own step), then sgm_paths and wta_hv once per
// sub-batch of tune::kBatchSubFrames frames.  The frames' census + cost
// kernels run on up to tune::kBatchCostStreams side streams forked from the
// context stream, in frame order per stream; the context stream starts a
// sub-batch's aggregation as soon as that sub-batch's costs are done, so the
// next sub-batches' (VALU-bound, small) cost kernels overlap the current
// (HBM-bound) aggregation.  jobs[0..n) share D, dmin, P1, P2 and subpixel
// (checked by the entry point); maps / sub hold n planes of W*H.
// cf set (sva_disparity_sgm_batch_conf_d): wta_hv's confidence instance, its
// planes n frames like maps; each sub-batch's launch gets them offset here and
// the kernel offsets them per frame.  fail_at: SVA_DEBUG_FAIL_COST_AT as the
// entry point read it.
int run_sgm_batch(Ctx* c, const sva_pair_d* jobs, int n, int W, int H, size_t pitch,
                  uint16_t* maps, float* sub, const ConfOut* cf, int fail_at) {
    const sva_sgm_params* p = &jobs[0].params;
    const int Dp = padded_D(p->D);
    const size_t np = (size_t)W * H, nv = np * (size_t)Dp;
    const int sb = tune::kBatchSubFrames > 0 ? std::min(n, tune::kBatchSubFrames) : n;
    const int nsub = (n + sb - 1) / sb;
    SVA_HIP(c, c->cost.ensure(nv * n), "cost workspace");
    // the aggregation workspaces serve one sub-batch at a time (same stream):
    // full sub-batches of sb frames, then the rest
    const AggPlan full = batch_plan(agg_shape(W, H, Dp, p), sb);
    const AggPlan rest = batch_plan(agg_shape(W, H, Dp, p), n - (nsub - 1) * sb);
    SVA_HIP(c, c->paths.ensure(full.paths_bytes), "path workspace");
    SVA_HIP(c, c->ckpt.ensure(full.ckpt_bytes), "checkpoint workspace");
    uint8_t* C = (uint8_t*)c->cost.ptr;
    const int ns = std::min(n, tune::kBatchCostStreams);
    if (ns > 1) {
        while ((int)c->side.size() < ns) {
            hipStream_t s = nullptr;
            SVA_HIP(c, hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "side stream");
            c->side.push_back(s);
        }
        // one event per (sub-batch, side stream): "this stream's frames of
        // sub-batch j have their cost volumes"
        while ((int)c->side_done.size() < ns * nsub) {
            hipEvent_t e = nullptr;
            SVA_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming), "side stream event");
            c->side_done.push_back(e);
        }
        if (!c->fork) SVA_HIP(c, hipEventCreateWithFlags(&c->fork, hipEventDisableTiming), "fork event");
        SVA_HIP(c, hipEventRecord(c->fork, c->stream), "fork");
        for (int s = 0; s < ns; s++) SVA_HIP(c, hipStreamWaitEvent(c->side[s], c->fork, 0), "fork");
    }
    SVA_HIP(c, c->census_side.ensure(np * 16 * (size_t)std::max(ns, 1)), "census workspace");
    const hipStream_t own = c->stream;
    // fault injection (SVA_DEBUG_FAIL_COST_AT): this call's fail_at-th cost launch fails
    int st = SVA_OK;
    for (int i = 0; i < n && st == SVA_OK; i++) {
        const sva_sgm_params* q = &jobs[i].params;
        uint8_t* Ci = C + (size_t)i * nv;
        if (ns > 1) c->stream = c->side[i % ns];
        // (the split route's census maps: this side stream's slot)
        uint64_t* cl = (uint64_t*)c->census_side.ptr + (size_t)(i % std::max(ns, 1)) * 2 * np;
        hipError_t e = i + 1 == fail_at
                           ? hipErrorLaunchFailure
                           : form_cost(*c, cost_route(Dp, q->dir, q->dir_y), jobs[i].left,
                                       jobs[i].right, W, H, pitch, Dp, q, q->dir, q->dir_y, Ci, cl,
                                       cl + np, true);
        // the last frame of a sub-batch on this side stream (or of the batch)
        if (e == hipSuccess && ns > 1 && (i + ns >= n || (i + ns) / sb != i / sb))
            e = hipEventRecord(c->side_done[(size_t)(i / sb) * ns + i % ns], c->stream);
        c->stream = own;
        if (e != hipSuccess) st = hip_fail(c, e, "cost launch");
    }
    // Aggregation per sub-batch on the context stream, after its costs.
    for (int j = 0; j < nsub && st == SVA_OK; j++) {
        const int i0 = j * sb, m = std::min(sb, n - i0);
        hipError_t e = hipSuccess;
        if (ns > 1) {
            for (int s = 0; s < ns && s < n && e == hipSuccess; s++) {
                // side stream s holds frames of sub-batch j: its event recorded
                // after the last of them
                bool has = false;
                for (int i = i0; i < i0 + m; i++) has = has || i % ns == s;
                if (has) e = hipStreamWaitEvent(c->stream, c->side_done[(size_t)j * ns + s], 0);
            }
        }
        if (e != hipSuccess) { st = hip_fail(c, e, "join"); break; }
        const AggPlan& plan = m == sb ? full : rest;
        const AggBuffers b = carve(plan, C + (size_t)i0 * nv, c->paths.ptr, c->ckpt.ptr);
        if ((e = launch_paths(*c, plan, b)) != hipSuccess) {
            st = hip_fail(c, e, "paths launch");
            break;
        }
        const ConfOut cfj = conf_at(cf, (size_t)i0 * np);
        if ((e = launch_wta_hv(*c, plan, b, maps + (size_t)i0 * np,
                               p->subpixel && sub ? sub + (size_t)i0 * np : nullptr,
                               cf ? &cfj : nullptr)) != hipSuccess) {
            st = hip_fail(c, e, "wta launch");
            break;
        }
    }
    if (st != SVA_OK && ns > 1) {
        // A failed launch skipped later sub-batches' joins, so the context
        // stream may not be ordered after cost kernels already queued on the
        // side streams.  Join every side stream with a fresh record before
        // returning: the caller may free or reuse the images and the cost
        // workspace as soon as the context stream has drained.  (side_done[s]
        // is free for this: nothing later in this call waits on it.)
        for (int s = 0; s < ns; s++) {
            if (hipEventRecord(c->side_done[s], c->side[s]) != hipSuccess ||
                hipStreamWaitEvent(c->stream, c->side_done[s], 0) != hipSuccess)
                (void)hipStreamSynchronize(c->side[s]);   // last resort: order on the host
        }
    }
    return st;
}

int check_camera(Ctx* c, const sva_camera* cam) {
    if (!cam) return fail(c, SVA_ERR_INVALID_ARG, "null camera");
    return SVA_OK;
}

int run_ref_device(Ctx* c, const uint8_t* ref, const uint8_t* other, int W, int H, size_t pitch,
                   const uint8_t* mask, const sva_camera* cref, const sva_camera* coth, int k,
                   double t_near, double t_far, uint8_t* d8, uint16_t* d16, uint8_t* valid) {
    const size_t np = (size_t)W * H;
    SVA_HIP(c, c->census_l.ensure(np * 16), "endpoint workspace");
    SVA_HIP(c, c->census_r.ensure(np), "endpoint workspace");
    int32_t* ends = (int32_t*)c->census_l.ptr;
    uint8_t* ok = (uint8_t*)c->census_r.ptr;
    SVA_HIP(c, launch_ref_endpoints(*c, W, H, *cref, *coth, k, t_near, t_far, ends, ok),
            "endpoint launch");
    SVA_HIP(c, launch_ref_match(*c, ref, other, W, H, pitch, mask, ends, ok, k, d8, d16, valid),
            "match launch");
    return SVA_OK;
}

int check_ref_args(Ctx* c, int W, int H, int k, double t_near, double t_far) {
    if (k < 1) return fail(c, SVA_ERR_INVALID_ARG, "kernel half-size k must be >= 1");
    if (2LL * k >= W || 2LL * k >= H) return fail(c, SVA_ERR_INVALID_ARG, "image smaller than window");
    if (!(t_near > 0.0) || !(t_far > 0.0))
        return fail(c, SVA_ERR_INVALID_ARG, "ray parameters must be positive");
    // the plane kernel packs line geometry in 16-bit fields (ref_line.h)
    if (W > 32767 || H > 32767)
        return fail(c, SVA_ERR_UNSUPPORTED, "Mode R supports W, H <= 32767");
    return SVA_OK;
}

// refinement / 3-D helpers

int check_planes(Ctx* c, int W, int H, size_t pitch) {
    if (W <= 0 || H <= 0) return fail(c, SVA_ERR_INVALID_ARG, "image size must be positive");
    if (pitch < (size_t)W) return fail(c, SVA_ERR_INVALID_ARG, "pitch smaller than width");
    if ((long long)W * H > (1ll << 31) - 1) return fail(c, SVA_ERR_INVALID_ARG, "image too large");
    if (H > 65535) return fail(c, SVA_ERR_UNSUPPORTED, "H must be <= 65535 (gridDim.y)");
    return SVA_OK;
}

int check_window(Ctx* c, int window_size) {
    if (window_size < 1) return fail(c, SVA_ERR_UNSUPPORTED, "window_size must be >= 1");
    return SVA_OK;
}

// improveWithDisparity on device planes; images = n device pointers.
int run_improve(Ctx* c, const uint8_t* disp, const uint8_t* center, const uint8_t* const* images,
                const sva_camera* cams, int n, int W, int H, size_t pitch, const uint8_t* mask,
                int window_size, int strict, uint8_t* out,
                const std::function<int(int, const uint8_t**)>& fetch) {
    const size_t bytes = (size_t)H * pitch;
    SVA_HIP(c, c->shifted.ensure(bytes), "shift workspace");
    SVA_HIP(c, c->total.ensure(sizeof(long long)), "fault flag");
    int* fault = (int*)c->total.ptr;
    SVA_HIP(c, hipMemsetAsync(fault, 0, sizeof(int), c->stream), "memset");
    uint8_t* sh = (uint8_t*)c->shifted.ptr;
    const int k = (window_size - 1) / 2;
    for (int i = 0; i < n; i++) {
        const uint8_t* img = images ? images[i] : nullptr;
        int s;
        if (fetch && (s = fetch(i, &img))) return s;
        // the reference's shifted Mat is uninitialised; DESIGN.md §2.7 fixes it to 0
        // (zero_fill: the shift kernel writes the 0 of every untouched pixel)
        SVA_HIP(c, launch_shift_perspective(*c, cams[2 * i], cams[2 * i + 1], disp, img, W, H,
                                            pitch, sh, true), "shift launch");
        SVA_HIP(c, launch_refine(*c, disp, center, sh, mask, W, H, pitch, k, cams[2 * i],
                                 cams[2 * i + 1], out, fault), "refine launch");
    }
    if (strict) {
        int f = 0;
        SVA_HIP(c, hipMemcpyAsync(&f, fault, sizeof(int), hipMemcpyDeviceToHost, c->stream),
                "download");
        SVA_HIP(c, hipStreamSynchronize(c->stream), "sync");
        if (f)
            return fail(c, SVA_ERR_INVALID_ARG,
                        "a masked pixel's window leaves the image (the reference's ROI throws)");
    }
    return SVA_OK;
}

int check_uniqueness(Ctx* c, int uniqueness) {
    if (uniqueness < 0 || uniqueness > 100)
        return fail(c, SVA_ERR_INVALID_ARG, "uniqueness must be 0..100 (percent, 0 = off)");
    return SVA_OK;
}

// Staging of the host-pointer entry points over the context's in_* / out_*
// buffers, everything on c->stream.  A step that fails leaves its status in
// st and turns the later steps into no-ops: an entry point stages its inputs,
// returns st if set, runs its _d twin's run function on the staged pointers,
// downloads and returns sync().
struct Staging {
    Ctx* c;
    int st = SVA_OK;
    void note(hipError_t e, const char* what) {
        if (e != hipSuccess) st = hip_fail(c, e, what);
    }
    // b grown to `bytes`: an output, or the destination of the uploads below
    template <class T>
    T* out(DevBuf& b, size_t bytes) {
        if (st == SVA_OK) note(b.ensure(bytes), "staging");
        return (T*)b.ptr;
    }
    template <class T>
    T* up(DevBuf& b, const void* src, size_t bytes) {
        T* d = out<T>(b, bytes);
        if (st == SVA_OK)
            note(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, c->stream), "upload");
        return d;
    }
    // H rows of W bytes, `pitch` apart at the caller's, packed on the device
    uint8_t* up2d(DevBuf& b, const uint8_t* src, size_t pitch, int W, int H) {
        uint8_t* d = out<uint8_t>(b, (size_t)W * H);
        if (st == SVA_OK)
            note(hipMemcpy2DAsync(d, W, src, pitch, W, H, hipMemcpyHostToDevice, c->stream),
                 "upload");
        return d;
    }
    // (an optional output the caller left out, dst null, is skipped)
    void down(void* dst, const void* src, size_t bytes) {
        if (st == SVA_OK && dst)
            note(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream), "download");
    }
    // rows of W bytes packed on the device, `pitch` apart at the caller's
    void down2d(void* dst, size_t pitch, const void* src, size_t W, size_t rows) {
        if (st == SVA_OK && dst)
            note(hipMemcpy2DAsync(dst, pitch, src, W, W, rows, hipMemcpyDeviceToHost, c->stream),
                 "download");
    }
    int sync() {
        if (st == SVA_OK) note(hipStreamSynchronize(c->stream), "sync");
        return st;
    }
};

}  // namespace

// ------------------------------------- the map filters --
// Behind the eight entries near the end of this file; a template, so outside extern "C".
namespace {

// A filter's workspace of `per` bytes for every pixel of the n maps, grown with
// its own out-of-memory report.
int filter_workspace(Ctx* c, DevBuf& ws, const MapArgs& m, size_t per, const char* name,
                     uint32_t** out) {
    const unsigned long long planes = (unsigned long long)m.W * m.H * (unsigned long long)m.n;
    if (planes > (~(size_t)0) / per)
        return fail(c, SVA_ERR_OUT_OF_MEMORY,
                    std::string(name) + " workspace: larger than the address space");
    const hipError_t e = ws.ensure((size_t)planes * per);
    if (e != hipSuccess) {
        (void)hipGetLastError();   // the failed allocation is reported here, not by a later call
        return fail(c, SVA_ERR_OUT_OF_MEMORY,
                    std::string(name) + " workspace: " + hipGetErrorString(e));
    }
    *out = (uint32_t*)ws.ptr;
    return SVA_OK;
}

// Each run_x: a checked call on device planes.
int run_cross(Ctx* c, const CrossArgs& a) {
    const MapArgs& m = a.m;
    const int order = c->dbg_cross_order >= 0 ? c->dbg_cross_order : tune::kCrossTileMajor;
    SVA_HIP(c, launch_cross_check(*c, m.disps, m.subpix, m.n, m.W, m.H, a.view_step, m.invalid,
                                  a.max_diff, a.min_agree, a.max_conflict, order, m.out, m.out_sub,
                                  a.agree, a.conflict),
            "cross-check launch");
    return SVA_OK;
}

// The label and count planes, then the launches.  max_size = 0 without comp_size
// is a copy and takes no workspace.
int run_speckle(Ctx* c, const SpeckleArgs& a) {
    const MapArgs& m = a.m;
    uint32_t *label = nullptr, *count = nullptr;
    if (a.max_size != 0 || a.comp_size) {
        if (int s = filter_workspace(c, c->speckle_ws, m, 8, "speckle", &label)) return s;
        count = label + (size_t)m.W * m.H * (size_t)m.n;
    }
    SVA_HIP(c, launch_speckle(*c, m.disps, m.subpix, m.n, m.W, m.H, m.invalid, a.max_size,
                              a.max_diff, label, count, m.out, m.out_sub, a.comp_size),
            "speckle launch");
    return SVA_OK;
}

// The key planes, then the launches.  max_dist = 0 is a copy and takes no workspace.
int run_fill(Ctx* c, const FillArgs& a) {
    const MapArgs& m = a.m;
    uint32_t* keys = nullptr;
    if (a.max_dist != 0)
        if (int s = filter_workspace(c, c->fill_ws, m, 32, "fill", &keys)) return s;
    const int segment = c->dbg_fill_segment > 0 ? c->dbg_fill_segment : tune::kFillSegment;
    SVA_HIP(c, launch_fill(*c, m.disps, m.subpix, m.n, m.W, m.H, m.invalid, a.max_dist, a.min_found,
                           a.mode, segment, keys, m.out, m.out_sub, a.n_found),
            "fill launch");
    return SVA_OK;
}

int run_wmed(Ctx* c, const WmedArgs& a) {
    const MapArgs& m = a.m;
    SVA_HIP(c, launch_wmedian(*c, m.disps, m.subpix, a.guides, a.guide_pitch, a.weights, a.select,
                              m.n, m.W, m.H, m.invalid, a.radius, a.min_support, a.fill, m.out,
                              m.out_sub, a.support),
            "wmed launch");
    return SVA_OK;
}

// The common planes of a host call on the device: the u16 maps through in_a and
// the f32 maps (sub_in: whether the filter takes them) through in_mask; in_place:
// the filter runs in place on them, else into out_a and out_b.  A host entry
// stages its own planes through g as well, runs run_x on the device form of its
// arguments, downloads its own planes and returns done().
struct StagedMaps {
    Staging g;
    const MapArgs& host;
    size_t nnp;
    MapArgs d;
    StagedMaps(Ctx* c, const MapArgs& m, bool in_place, bool sub_in)
        : g{c}, host(m), nnp((size_t)m.W * m.H * (size_t)m.n), d(m) {
        uint16_t* dd = g.up<uint16_t>(c->in_a, m.disps, nnp * 2);
        float* ds = sub_in ? g.up<float>(c->in_mask, m.subpix, nnp * 4) : nullptr;
        d.disps = dd;
        d.subpix = ds;
        d.out = in_place ? dd : g.out<uint16_t>(c->out_a, nnp * 2);
        d.out_sub = !m.out_sub ? nullptr : in_place ? ds : g.out<float>(c->out_b, nnp * 4);
    }
    int done() {
        g.down(host.out, d.out, nnp * 2);
        g.down(host.out_sub, d.out_sub, nnp * 4);
        return g.sync();
    }
};

// The count planes stage through out_c, agree first.
int cross_host(Ctx* c, const CrossArgs& a) {
    StagedMaps s(c, a.m, false, a.m.subpix != nullptr);
    uint8_t* cnt = a.agree || a.conflict ? s.g.out<uint8_t>(c->out_c, s.nnp * 2) : nullptr;
    CrossArgs d = a;
    d.m = s.d;
    d.agree = a.agree ? cnt : nullptr;
    d.conflict = a.conflict ? cnt + s.nnp : nullptr;
    if (s.g.st) return s.g.st;
    if (int st = run_cross(c, d)) return st;
    s.g.down(a.agree, d.agree, s.nnp);
    s.g.down(a.conflict, d.conflict, s.nnp);
    return s.done();
}

int speckle_host(Ctx* c, const SpeckleArgs& a) {
    StagedMaps s(c, a.m, true, a.m.out_sub != nullptr);
    SpeckleArgs d = a;
    d.m = s.d;
    d.comp_size = a.comp_size ? s.g.out<uint32_t>(c->out_c, s.nnp * 4) : nullptr;
    if (s.g.st) return s.g.st;
    if (int st = run_speckle(c, d)) return st;
    s.g.down(a.comp_size, d.comp_size, s.nnp * 4);
    return s.done();
}

int fill_host(Ctx* c, const FillArgs& a) {
    StagedMaps s(c, a.m, true, a.m.out_sub != nullptr);
    FillArgs d = a;
    d.m = s.d;
    d.n_found = a.n_found ? s.g.out<uint8_t>(c->out_c, s.nnp) : nullptr;
    if (s.g.st) return s.g.st;
    if (int st = run_fill(c, d)) return st;
    s.g.down(a.n_found, d.n_found, s.nnp);
    return s.done();
}

// select stages through in_c and support through out_c; the guides are packed
// on the device, one W x H image per map (weights stays the caller's host table).
int wmed_host(Ctx* c, const WmedArgs& a) {
    const MapArgs& m = a.m;
    StagedMaps s(c, m, false, m.out_sub != nullptr);
    const size_t np = (size_t)m.W * m.H;
    WmedArgs d = a;
    d.m = s.d;
    d.select = a.select ? s.g.up<uint8_t>(c->in_c, a.select, s.nnp) : nullptr;
    std::vector<const uint8_t*> dguides;
    if (a.guides) {
        uint8_t* dg = s.g.out<uint8_t>(c->wmed_guides, s.nnp);
        for (int i = 0; i < m.n && s.g.st == SVA_OK; i++) {
            s.g.note(hipMemcpy2DAsync(dg + (size_t)i * np, m.W, a.guides[i], a.guide_pitch, m.W,
                                      m.H, hipMemcpyHostToDevice, c->stream),
                     "upload");
            dguides.push_back(dg + (size_t)i * np);
        }
        d.guides = dguides.data();
    }
    d.guide_pitch = (size_t)m.W;
    d.support = a.support ? s.g.out<uint16_t>(c->out_c, s.nnp * 2) : nullptr;
    if (s.g.st) return s.g.st;
    if (int st = run_wmed(c, d)) return st;
    s.g.down(a.support, d.support, s.nnp * 2);
    return s.done();
}

int run_mask(Ctx* c, const MaskArgs& a) {
    const MapArgs& m = a.m;
    SVA_HIP(c, launch_mask_maps(*c, m.disps, m.subpix, a.valid, m.n, m.W, m.H, m.invalid, m.out,
                                m.out_sub),
            "mask launch");
    return SVA_OK;
}

// valid stages through in_c.
int mask_host(Ctx* c, const MaskArgs& a) {
    StagedMaps s(c, a.m, true, a.m.out_sub != nullptr);
    MaskArgs d = a;
    d.m = s.d;
    d.valid = s.g.up<uint8_t>(c->in_c, a.valid, s.nnp);
    if (s.g.st) return s.g.st;
    if (int st = run_mask(c, d)) return st;
    return s.done();
}

int run_rectify(Ctx* c, const RectifyArgs& a) {
    SVA_HIP(c, launch_rectify(*c, a.src, a.n, a.src_w, a.src_h, a.src_pitch, a.views, a.out_w,
                              a.out_h, a.out_pitch, a.border, a.out, a.valid, a.map),
            "rectify launch");
    return SVA_OK;
}

// The views are packed on the device: src through in_a, out through out_a, valid
// through out_c and map through out_b; the caller's pitches hold on the host only.
int rectify_host(Ctx* c, const RectifyArgs& a) {
    Staging g{c};
    const size_t rows_in = (size_t)a.n * a.src_h, rows_out = (size_t)a.n * a.out_h;
    const size_t nout = rows_out * a.out_w;
    RectifyArgs d = a;
    uint8_t* ds = g.out<uint8_t>(c->in_a, rows_in * a.src_w);
    if (g.st == SVA_OK)
        g.note(hipMemcpy2DAsync(ds, a.src_w, a.src, a.src_pitch, a.src_w, rows_in,
                                hipMemcpyHostToDevice, c->stream),
               "upload");
    d.src = ds;
    d.src_pitch = (size_t)a.src_w;
    d.out_pitch = (size_t)a.out_w;
    d.out = g.out<uint8_t>(c->out_a, nout);
    d.valid = a.valid ? g.out<uint8_t>(c->out_c, nout) : nullptr;
    d.map = a.map ? g.out<int32_t>(c->out_b, nout * 8) : nullptr;
    if (g.st) return g.st;
    if (int st = run_rectify(c, d)) return st;
    g.down2d(a.out, a.out_pitch, d.out, (size_t)a.out_w, rows_out);
    g.down2d(a.valid, a.out_pitch, d.valid, (size_t)a.out_w, rows_out);
    g.down(a.map, d.map, nout * 8);
    return g.sync();
}

// One entry: the context, the rules, then the call on device planes (host null)
// or on host planes.
template <class Args>
int filter_entry(void* ctx, const Args& a, int (*check)(const Args&, std::string&),
                 int (*run)(Ctx*, const Args&), int (*host)(Ctx*, const Args&)) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    std::string msg;
    if (int s = check(a, msg)) return fail(c, s, msg);
    return host ? host(c, a) : run(c, a);
}
}  // namespace

// ------------------------------------------------------------------ ABI --
extern "C" {

void sva_sgm_params_default(sva_sgm_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->D = 128;
    p->dmin = 0;
    p->dir = -1;
    p->P1 = 10;
    p->P2 = 120;
    p->subpixel = 0;
    p->lr_check = 0;
    p->lr_max_diff = 1;
    p->invalid = 0xffff;
}

int sva_abi_version(void) { return SVA_ABI_VERSION; }

int sva_device_count(int* count) {
    if (!count) return SVA_ERR_INVALID_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return SVA_OK;
}

const char* sva_status_string(int s) {
    switch (s) {
        case SVA_OK: return "ok";
        case SVA_ERR_INVALID_ARG: return "invalid argument";
        case SVA_ERR_UNSUPPORTED: return "unsupported configuration";
        case SVA_ERR_DEVICE: return "device error";
        case SVA_ERR_OUT_OF_MEMORY: return "out of device memory";
        case SVA_ERR_NO_DEVICE: return "no usable HIP device";
        default: return "unknown status";
    }
}

int sva_create(int device, void** out) {
    if (!out) return SVA_ERR_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return SVA_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return SVA_ERR_INVALID_ARG;
    if (hipSetDevice(device) != hipSuccess) return SVA_ERR_DEVICE;
    Ctx* c = new (std::nothrow) Ctx();
    if (!c) return SVA_ERR_OUT_OF_MEMORY;
    c->device = device;
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return SVA_ERR_DEVICE;
    }
    c->stream = c->own_stream;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->cu_count = prop.multiProcessorCount;
    *out = c;
    return SVA_OK;
}

int sva_destroy(void* ctx) {
    Ctx* c = as_ctx(ctx);
    if (!c) return SVA_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->batch_lane.reset();   // its streams and staging (multi.cpp), before the context's own
    for (hipStream_t s : c->side) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    for (hipEvent_t e : c->side_done) (void)hipEventDestroy(e);
    if (c->fork) (void)hipEventDestroy(c->fork);
    c->census_side.release();
    for (DevBuf* b : {&c->census_l, &c->census_r, &c->cost, &c->paths, &c->ckpt, &c->scratch_u16,
                      &c->disp_r, &c->in_a, &c->in_b, &c->in_mask, &c->out_a, &c->out_b,
                      &c->out_c, &c->in_c, &c->shifted, &c->keys, &c->counts, &c->total, &c->ref_keys, &c->refine_ws, &c->speckle_ws, &c->fill_ws, &c->wmed_guides})
        b->release();
    c->timer.release_all();
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return SVA_OK;
}

int sva_set_stream(void* ctx, void* stream) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    c->stream = stream ? (hipStream_t)stream : c->own_stream;
    return SVA_OK;
}

int sva_synchronize(void* ctx) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    SVA_HIP(c, hipStreamSynchronize(c->stream), "hipStreamSynchronize");
    return SVA_OK;
}

const char* sva_last_error(void* ctx) {
    Ctx* c = as_ctx(ctx);
    return c ? c->last_error.c_str() : "null context";
}

namespace {

// The path kernel's time (ns, best of 3 after one warm-up launch) on the
// context's current cost / path / checkpoint buffers.  The volumes hold
// whatever they hold: the kernel's work does not depend on the values.
int time_stage_set(Ctx* c, int W, int H, int D, int64_t* ns) {
    // (the plan of a frame with the default penalties)
    const AggPlan plan = frame_plan(AggShape{W, H, D, 0, 10, 120}, tune::kDiagPairMinPixels);
    const AggBuffers buf = carve(plan, (const uint8_t*)c->cost.ptr, c->paths.ptr, c->ckpt.ptr);
    hipEvent_t a = nullptr, b = nullptr;
    SVA_HIP(c, hipEventCreate(&a), "placement event");
    if (hipEventCreate(&b) != hipSuccess) {
        (void)hipEventDestroy(a);
        return fail(c, SVA_ERR_DEVICE, "placement event");
    }
    hipError_t e = hipSuccess;
    float best = 0.f;
    for (int r = 0; r < 4 && e == hipSuccess; r++) {
        e = hipEventRecord(a, c->stream);
        if (e == hipSuccess) e = launch_paths(*c, plan, buf);
        if (e == hipSuccess) e = hipEventRecord(b, c->stream);
        if (e == hipSuccess) e = hipEventSynchronize(b);
        float ms = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
        if (e == hipSuccess && r > 0) best = r == 1 ? ms : std::min(best, ms);
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    if (e != hipSuccess) return hip_fail(c, e, "placement timing");
    *ns = (int64_t)((double)best * 1e6);
    return SVA_OK;
}

// sva_reserve's placement check (include/sva.h): keep the
// fastest of `trials` allocations of the stage buffers.  Every trial set stays
// allocated until the choice is made, so each one lands on pages no earlier
// set holds; a trial is taken only while the device keeps a quarter of its
// memory (at least 16 GiB) free beside it.
int place_stage_buffers(Ctx* c, int W, int H, int D, int trials) {
    struct Set {
        DevBuf cost, paths, ckpt;
        int64_t ns = 0;
    };
    const bool timing = c->timer.enabled;
    c->timer.enabled = false;                 // the trials are not the caller's launches
    std::vector<Set> sets(1);
    int rc = time_stage_set(c, W, H, D, &sets[0].ns);
    const size_t set_bytes = c->cost.bytes + c->paths.bytes + c->ckpt.bytes;
    for (int t = 1; rc == SVA_OK && t < trials; t++) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) break;
        const size_t keep = std::max(total_b / 4, (size_t)16 << 30);
        if (free_b < set_bytes + keep) break;
        Set n;
        n.cost.flags = c->cost.flags;
        n.paths.flags = c->paths.flags;
        n.ckpt.flags = c->ckpt.flags;
        if (n.cost.ensure(c->cost.bytes) != hipSuccess || n.paths.ensure(c->paths.bytes) != hipSuccess ||
            n.ckpt.ensure(c->ckpt.bytes) != hipSuccess) {
            n.cost.release();                 // no room for another set: stop here
            n.paths.release();
            n.ckpt.release();
            (void)hipGetLastError();
            break;
        }
        // time the new set in the context's slots; sets[0] keeps the first set
        std::swap(c->cost, n.cost);
        std::swap(c->paths, n.paths);
        std::swap(c->ckpt, n.ckpt);
        rc = time_stage_set(c, W, H, D, &n.ns);
        std::swap(c->cost, n.cost);
        std::swap(c->paths, n.paths);
        std::swap(c->ckpt, n.ckpt);
        sets.push_back(n);
    }
    c->timer.enabled = timing;
    size_t best = 0;
    int64_t worst = sets[0].ns;
    for (size_t i = 1; i < sets.size(); i++) {
        if (sets[i].ns < sets[best].ns) best = i;
        worst = std::max(worst, sets[i].ns);
    }
    if (rc == SVA_OK && best != 0) {          // the context takes the fastest set
        std::swap(c->cost, sets[best].cost);
        std::swap(c->paths, sets[best].paths);
        std::swap(c->ckpt, sets[best].ckpt);
    }
    const int64_t kept = sets[rc == SVA_OK ? best : 0].ns;
    for (size_t i = 1; i < sets.size(); i++) {  // every other set (the old slots included)
        sets[i].cost.release();
        sets[i].paths.release();
        sets[i].ckpt.release();
    }
    if (rc != SVA_OK) return rc;
    c->placement_ns = kept;
    c->placement_worst_ns = worst;
    c->placement_paths = c->paths.ptr;
    return SVA_OK;
}

}  // namespace

int sva_reserve(void* ctx, int W, int H, int D) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    if (W <= 0 || H <= 0 || D <= 0) return fail(c, SVA_ERR_INVALID_ARG, "bad reserve size");
    if (padded_D(D)) D = padded_D(D);     // a frame's volumes use the native width (§4.7)
    const size_t np = (size_t)W * H, nv = np * (size_t)D;
    SVA_HIP(c, c->census_l.ensure(np * 8), "reserve");
    SVA_HIP(c, c->census_r.ensure(np * 8), "reserve");
    SVA_HIP(c, c->cost.ensure(nv), "reserve");
    // the frame route's workspaces, for either diagonal route (tile pipeline)
    const AggReserve r = reserve_plan(W, H, D);
    SVA_HIP(c, c->paths.ensure(r.paths_bytes), "reserve");
    SVA_HIP(c, c->ckpt.ensure(r.ckpt_bytes), "reserve");
    // (once per allocation: a repeated reserve of a size the buffers already
    // hold keeps the set the last check chose)
    const int trials = c->placement_trials > 0 ? c->placement_trials : tune::kPlacementTrials;
    if (trials > 1 && is_native_d(D) && nv < ((size_t)1 << 32) &&
        nv + r.paths_bytes + r.ckpt_bytes >= tune::kPlacementMinBytes && c->paths.ptr != c->placement_paths)
        return place_stage_buffers(c, W, H, D, trials);
    return SVA_OK;
}

int sva_set_path_kernel(void* ctx, int kernel) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    if (kernel == SVA_PATH_KERNEL_FUSED)
        return fail(c, SVA_ERR_UNSUPPORTED,
                    "the census-fused path kernel was removed in ABI v4 (DESIGN.md §4.5)");
    if (kernel != SVA_PATH_KERNEL_COST_VOLUME && kernel != SVA_PATH_KERNEL_AUTO)
        return fail(c, SVA_ERR_INVALID_ARG, "unknown path kernel");
    return SVA_OK;
}

int sva_set_timing(void* ctx, int enable) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    if (enable < 0 || enable > SVA_TIMING_AGG)
        return fail(c, SVA_ERR_INVALID_ARG, "timing mode must be 0, 1, 2 or 3");
    c->timer.enabled = enable != 0;
    c->timer.mode = enable;
    return SVA_OK;
}

int sva_reset_timing(void* ctx) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    hipError_t e = c->timer.resolve();
    c->timer.totals.clear();
    if (e != hipSuccess) return hip_fail(c, e, "timer resolve");
    return SVA_OK;
}

int sva_set_debug(void* ctx, int key, int64_t value) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    switch (key) {
        case SVA_DEBUG_PLANE_SPLIT:
            if (value < 0 || value > 16) return fail(c, SVA_ERR_INVALID_ARG, "plane split must be 0..16");
            c->dbg_plane_split = (int)value;
            return SVA_OK;
        case SVA_DEBUG_FAIL_COST_AT:
            if (value < 0 || value > (1 << 30)) return fail(c, SVA_ERR_INVALID_ARG, "bad frame index");
            c->dbg_fail_cost_at = (int)value;
            return SVA_OK;
        case SVA_DEBUG_PLACEMENT_TRIALS:
            if (value < 0 || value > 8) return fail(c, SVA_ERR_INVALID_ARG, "placement trials must be 0..8");
            c->placement_trials = (int)value;
            return SVA_OK;
        case SVA_DEBUG_DIAG_PAIR_MIN_PIXELS:
            if (value < -1) return fail(c, SVA_ERR_INVALID_ARG, "pair route threshold must be >= -1");
            c->dbg_pair_min_pixels = value;
            return SVA_OK;
        case SVA_DEBUG_REFINE_ROUTE:
            if (value < 0 || value > 1) return fail(c, SVA_ERR_INVALID_ARG, "refine route must be 0 or 1");
            c->dbg_refine_route = (int)value;
            return SVA_OK;
        case SVA_DEBUG_CROSS_ORDER:
            if (value < -1 || value > 1)
                return fail(c, SVA_ERR_INVALID_ARG, "cross order must be -1, 0 or 1");
            c->dbg_cross_order = (int)value;
            return SVA_OK;
        case SVA_DEBUG_FILL_SEGMENT:
            if (value < 0 || value > 65536)
                return fail(c, SVA_ERR_INVALID_ARG, "fill segment must be 0..65536");
            c->dbg_fill_segment = (int)value;
            return SVA_OK;
        default:
            return fail(c, SVA_ERR_INVALID_ARG, "unknown or read-only debug key");
    }
}

int sva_get_debug(void* ctx, int key, int64_t* value) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    if (!value) return fail(c, SVA_ERR_INVALID_ARG, "null value");
    switch (key) {
        case SVA_DEBUG_PLANE_SPLIT: *value = c->dbg_plane_split; return SVA_OK;
        case SVA_DEBUG_FAIL_COST_AT: *value = c->dbg_fail_cost_at; return SVA_OK;
        case SVA_DEBUG_PLACEMENT_TRIALS: *value = c->placement_trials; return SVA_OK;
        case SVA_DEBUG_PLACEMENT_NS: *value = c->placement_ns; return SVA_OK;
        case SVA_DEBUG_PLACEMENT_WORST_NS: *value = c->placement_worst_ns; return SVA_OK;
        case SVA_DEBUG_DIAG_ROUTE: *value = c->last_diag_route; return SVA_OK;
        case SVA_DEBUG_DIAG_PAIR_MIN_PIXELS:
            *value = c->dbg_pair_min_pixels >= 0 ? c->dbg_pair_min_pixels : (int64_t)tune::kDiagPairMinPixels;
            return SVA_OK;
        case SVA_DEBUG_REFINE_ROUTE: *value = c->dbg_refine_route; return SVA_OK;
        case SVA_DEBUG_REFINE_LAST_ROUTE: *value = c->last_refine_route; return SVA_OK;
        case SVA_DEBUG_CROSS_ORDER:
            *value = c->dbg_cross_order >= 0 ? c->dbg_cross_order : tune::kCrossTileMajor;
            return SVA_OK;
        case SVA_DEBUG_FILL_SEGMENT:
            *value = c->dbg_fill_segment > 0 ? c->dbg_fill_segment : tune::kFillSegment;
            return SVA_OK;
        case SVA_DEBUG_SIDE_IDLE: {
            bool idle = true;
            for (hipStream_t s : c->side) {
                const hipError_t e = hipStreamQuery(s);
                if (e == hipErrorNotReady) idle = false;
                else if (e != hipSuccess) return hip_fail(c, e, "side stream query");
            }
            *value = idle ? 1 : 0;
            return SVA_OK;
        }
        default:
            return fail(c, SVA_ERR_INVALID_ARG, "unknown debug key");
    }
}

int sva_kernel_time(void* ctx, const char* name, double* total_ms, int64_t* count) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    if (!name || !total_ms || !count) return fail(c, SVA_ERR_INVALID_ARG, "null argument");
    hipError_t e = c->timer.resolve();
    if (e != hipSuccess) return hip_fail(c, e, "timer resolve");
    auto it = c->timer.totals.find(name);
    *total_ms = it == c->timer.totals.end() ? 0.0 : it->second.first;
    *count = it == c->timer.totals.end() ? 0 : it->second.second;
    return SVA_OK;
}

// ---------------------------------------------------------------- Mode S --
namespace {
// Arguments of sva_disparity_sgm[_conf][_d]; the plain forms pass uniqueness 0.
int check_sgm_frame(Ctx* c, const uint8_t* left, const uint8_t* right, int W, int H, size_t pitch,
                    const sva_sgm_params* p, int uniqueness, const uint16_t* disp) {
    int s;
    if ((s = check_image(c, left, W, H, pitch)) || (s = check_image(c, right, W, H, pitch)) ||
        (s = check_sgm(c, p, W, H)) || (s = check_uniqueness(c, uniqueness)))
        return s;
    if (!disp) return fail(c, SVA_ERR_INVALID_ARG, "null disparity output");
    return SVA_OK;
}

// The host-buffer forms of Mode S: sva_disparity_sgm (conf false) and
// sva_disparity_sgm_conf, which adds the WTA's confidence planes and the
// uniqueness filter.
int sgm_host(void* ctx, const uint8_t* left, const uint8_t* right, int W, int H, size_t pitch,
             const sva_sgm_params* p, bool conf, int uniqueness, uint16_t* disp, float* sub,
             uint16_t* cost_min, uint16_t* cost_second) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_sgm_frame(c, left, right, W, H, pitch, p, uniqueness, disp))) return s;
    const bool want_sub = p->subpixel && sub;
    const size_t np = (size_t)W * H;
    Staging g{c};
    const uint8_t* dl = g.up2d(c->in_a, left, pitch, W, H);
    const uint8_t* dr = g.up2d(c->in_b, right, pitch, W, H);
    uint16_t* dd = g.out<uint16_t>(c->out_a, np * 2);
    float* ds = want_sub ? g.out<float>(c->out_b, np * 4) : nullptr;
    // the two cost planes share one staging buffer
    uint16_t* dc = cost_min || cost_second ? g.out<uint16_t>(c->out_c, np * 4) : nullptr;
    if (g.st) return g.st;
    const ConfOut cf{cost_min ? dc : nullptr, cost_second ? dc + np : nullptr, uniqueness,
                     p->invalid};
    if ((s = run_sgm_device(c, dl, dr, W, H, W, p, dd, ds, conf ? &cf : nullptr))) return s;
    g.down(disp, dd, np * 2);
    if (want_sub) g.down(sub, ds, np * 4);
    g.down(cost_min, cf.cost_min, np * 2);
    g.down(cost_second, cf.cost_second, np * 2);
    return g.sync();
}

// The batch entry points: sva_disparity_sgm_batch_d (cf null) and its
// confidence form.
int sgm_batch_d(void* ctx, const sva_pair_d* jobs, int n, int W, int H, size_t pitch,
                uint16_t* maps, float* sub, const ConfOut* cf) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    // SVA_DEBUG_FAIL_COST_AT is for "the next call": read and cleared before
    // validation, so that a call refused below does not leave it armed
    const int fail_at = c->dbg_fail_cost_at;
    c->dbg_fail_cost_at = 0;
    if (!jobs || n <= 0 || !maps) return fail(c, SVA_ERR_INVALID_ARG, "bad batch argument");
    int s;
    if (cf && (s = check_uniqueness(c, cf->uniqueness))) return s;
    const sva_sgm_params* p0 = &jobs[0].params;
    for (int i = 0; i < n; i++) {
        const sva_sgm_params* q = &jobs[i].params;
        if ((s = check_image(c, jobs[i].left, W, H, pitch)) ||
            (s = check_image(c, jobs[i].right, W, H, pitch)) || (s = check_sgm(c, q, W, H)))
            return s;
        if (q->D != p0->D || q->dmin != p0->dmin || q->P1 != p0->P1 || q->P2 != p0->P2 ||
            q->subpixel != p0->subpixel)
            return fail(c, SVA_ERR_INVALID_ARG,
                        "a batch's pairs must share D, dmin, P1, P2 and subpixel");
        // the filter writes one `invalid` per launch
        if (cf && q->invalid != p0->invalid)
            return fail(c, SVA_ERR_INVALID_ARG, "a confidence batch's pairs must share invalid");
        if (q->lr_check) return fail(c, SVA_ERR_UNSUPPORTED, "the batch route has no L/R check");
    }
    if (!is_native_d(padded_D(p0->D)))
        return fail(c, SVA_ERR_UNSUPPORTED, "no tile pipeline for this D");
    // chunks of at most tune::kBatchMaxPairs frames, whose workspaces stay
    // under tune::kBatchMaxBytes
    const int Dp = padded_D(p0->D);
    const size_t np = (size_t)W * H;
    const AggPlan one = batch_plan(agg_shape(W, H, Dp, p0), 1);
    const size_t per = one.vol + one.paths_bytes + one.ckpt_bytes;
    int chunk = tune::kBatchMaxPairs;
    while (chunk > 1 && per * (size_t)chunk > tune::kBatchMaxBytes) chunk--;
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const ConfOut cfi = conf_at(cf, (size_t)i0 * np);
        // (the injected failure counts the first chunk's launches, as before)
        if ((s = run_sgm_batch(c, jobs + i0, std::min(chunk, n - i0), W, H, pitch,
                               maps + (size_t)i0 * np, sub ? sub + (size_t)i0 * np : nullptr,
                               cf ? &cfi : nullptr, i0 == 0 ? fail_at : 0)))
            return s;
    }
    return SVA_OK;
}

// The steps of the multi-baseline entry points: n in 1..32 nonzero steps.
int check_steps(Ctx* c, const int32_t* steps, int n) {
    if (n < 1 || n > 32) return fail(c, SVA_ERR_INVALID_ARG, "n must be 1..32 matched images");
    if (!steps) return fail(c, SVA_ERR_INVALID_ARG, "null steps");
    for (int i = 0; i < n; i++) {
        const int sx = steps[2 * i], sy = steps[2 * i + 1];
        if (sx < -255 || sx > 255 || sy < -255 || sy > 255 || (sx == 0 && sy == 0))
            return fail(c, SVA_ERR_INVALID_ARG, "every step must be nonzero, |comp| <= 255");
    }
    return SVA_OK;
}

// Arguments of sva_disparity_sgm_multi[_d]; nothing is launched before they pass.
int check_sgm_multi(Ctx* c, const uint8_t* ref, const uint8_t* const* others, const int32_t* steps,
                    int n, int W, int H, size_t pitch, const sva_sgm_params* p, int uniqueness,
                    const uint16_t* disp) {
    int s;
    if (!p) return fail(c, SVA_ERR_INVALID_ARG, "null params");
    if ((s = check_steps(c, steps, n))) return s;
    if (!others) return fail(c, SVA_ERR_INVALID_ARG, "null image list");
    if ((s = check_image(c, ref, W, H, pitch))) return s;
    for (int i = 0; i < n; i++)
        if ((s = check_image(c, others[i], W, H, pitch))) return s;
    sva_sgm_params q = *p;   // (dir, dir_y) of the params are ignored: the steps stand in
    q.dir = steps[0];
    q.dir_y = steps[1];
    q.lr_check = 0;
    if ((s = check_sgm(c, &q, W, H)) || (s = check_uniqueness(c, uniqueness))) return s;
    if (p->lr_check)
        return fail(c, SVA_ERR_UNSUPPORTED, "the multi-baseline route has no L/R check");
    if (!disp) return fail(c, SVA_ERR_INVALID_ARG, "null disparity output");
    if (!is_native_d(padded_D(p->D)))
        return fail(c, SVA_ERR_UNSUPPORTED, "no tile pipeline for this D");
    return SVA_OK;
}

// The baseline ratios of the mixed entry points: n (num, den)
// pairs in 1..8, reduced by their gcd into red[2n].  dmin >= 0 and D > 0 set
// the distance limit t(dmin + D - 1) <= 65535 (D = 0: no limit to check).
int check_ratios(Ctx* c, const int32_t* ratios, int n, int dmin, int D, int32_t* red) {
    if (!ratios) return fail(c, SVA_ERR_INVALID_ARG, "null ratios");
    for (int i = 0; i < n; i++) {
        int num = ratios[2 * i], den = ratios[2 * i + 1];
        if (num < 1 || num > mb::kMaxRatio || den < 1 || den > mb::kMaxRatio)
            return fail(c, SVA_ERR_INVALID_ARG, "every ratio needs num and den in 1..8");
        int a = num, b = den;
        while (b) { const int r = a % b; a = b; b = r; }
        red[2 * i] = num /= a;
        red[2 * i + 1] = den /= a;
        if (D > 0 && mb::mixed_distance(dmin + D - 1, num, den) > 65535)
            return fail(c, SVA_ERR_INVALID_ARG,
                        "the match distance (dmin + D - 1) * num / den must fit 16 bits");
    }
    return SVA_OK;
}

// Multi-baseline Mode S on device buffers: pair i's
// cost volume (ref against others[i] along steps[i]) into slot i of the cost
// workspace, cost_fuse into slot n, then the frame's aggregation and WTA on the
// fused volume.  The workspace holds n + 1 volumes.  ratios: null (equal
// baselines) or n reduced (num, den); a pair at 1/1 takes the frame's own cost
// route, every other pair census + cost_mixed.
int run_sgm_multi_device(Ctx* c, const uint8_t* ref, const uint8_t* const* others,
                         const int32_t* steps, const int32_t* ratios, int n, int W, int H,
                         size_t pitch, const sva_sgm_params* p, uint16_t* disp, float* sub,
                         const ConfOut* cf) {
    const int Dp = padded_D(p->D);
    const size_t np = (size_t)W * H, nv = np * (size_t)Dp;
    auto unit = [&](int i) { return !ratios || (ratios[2 * i] == 1 && ratios[2 * i + 1] == 1); };
    bool mixed = false;
    for (int i = 0; i < n; i++) mixed = mixed || !unit(i);
    SVA_HIP(c, c->cost.ensure(nv * ((size_t)n + 1)), "cost workspace");
    uint8_t* C = (uint8_t*)c->cost.ptr;
    // The pairs' cost kernels run one after another on the context stream: each
    // fills the chip, and spreading them over side streams measured no faster
    // (DESIGN.md §4.19).
    uint64_t *cl = nullptr, *cr = nullptr;
    auto census_maps = [&]() -> hipError_t {
        if (cl) return hipSuccess;
        hipError_t e = c->census_l.ensure(np * 8);
        if (e == hipSuccess) e = c->census_r.ensure(np * 8);
        cl = (uint64_t*)c->census_l.ptr;
        cr = (uint64_t*)c->census_r.ptr;
        return e;
    };
    for (int i = 0; i < n; i++) {
        if (!unit(i)) continue;
        const int sx = steps[2 * i], sy = steps[2 * i + 1];
        const CostRoute route = cost_route(Dp, sx, sy);
        if (route == CostRoute::Split) SVA_HIP(c, census_maps(), "census workspace");
        const char* what = "cost launch";
        const hipError_t e = form_cost(*c, route, ref, others[i], W, H, pitch, Dp, p, sx, sy,
                                       C + (size_t)i * nv, cl, cr, true, &what);
        if (e != hipSuccess) return hip_fail(c, e, what);
    }
    // The other pairs, after every unit pair: a split-route unit pair fills both
    // census maps itself, so the reference map that the mixed pairs share is
    // formed only once none of those is left to run (one stream: in order).
    if (mixed) {
        SVA_HIP(c, census_maps(), "census workspace");
        SVA_HIP(c, launch_census(*c, ref, W, H, pitch, cl), "census launch");
    }
    for (int i = 0; i < n; i++) {
        if (unit(i)) continue;
        SVA_HIP(c, launch_census(*c, others[i], W, H, pitch, cr), "census launch");
        SVA_HIP(c, launch_cost_mixed(*c, cl, cr, W, H, Dp, p->dmin, steps[2 * i], steps[2 * i + 1],
                                     ratios[2 * i], ratios[2 * i + 1], C + (size_t)i * nv, p->D),
                "cost launch");
    }
    // a group whose ratios are all 1/1 is an equal-baseline group
    uint8_t* Cf = C + (size_t)n * nv;
    SVA_HIP(c,
            launch_cost_fuse(*c, C, nv, n, W, H, Dp, p->D, p->dmin, steps, mixed ? ratios : nullptr,
                             Cf),
            "fuse launch");
    return paths_wta(c, Cf, W, H, p, Dp, disp, sub, cf);
}

// sva_disparity_sgm_multi_d (mixed false: ratios unused) and
// sva_disparity_sgm_mixed_d (mixed true: ratios checked and reduced).
int sgm_multi_d(void* ctx, const uint8_t* ref, const uint8_t* const* others, const int32_t* steps,
                const int32_t* ratios, bool mixed, int n, int W, int H, size_t pitch,
                const sva_sgm_params* p, int uniqueness, uint16_t* disp, float* sub,
                uint16_t* cost_min, uint16_t* cost_second) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_sgm_multi(c, ref, others, steps, n, W, H, pitch, p, uniqueness, disp))) return s;
    int32_t red[64];
    if (mixed && (s = check_ratios(c, ratios, n, p->dmin, p->D, red))) return s;
    const ConfOut cf{cost_min, cost_second, uniqueness, p->invalid};
    const bool conf = cost_min || cost_second || uniqueness;
    return run_sgm_multi_device(c, ref, others, steps, mixed ? red : nullptr, n, W, H, pitch, p,
                                disp, p->subpixel ? sub : nullptr, conf ? &cf : nullptr);
}

// The same from host images: sva_disparity_sgm_multi and sva_disparity_sgm_mixed.
int sgm_multi_host(void* ctx, const uint8_t* ref, const uint8_t* const* others,
                   const int32_t* steps, const int32_t* ratios, bool mixed, int n, int W, int H,
                   size_t pitch, const sva_sgm_params* p, int uniqueness, uint16_t* disp,
                   float* sub, uint16_t* cost_min, uint16_t* cost_second) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_sgm_multi(c, ref, others, steps, n, W, H, pitch, p, uniqueness, disp))) return s;
    int32_t red[64];
    if (mixed && (s = check_ratios(c, ratios, n, p->dmin, p->D, red))) return s;
    const bool want_sub = p->subpixel && sub;
    const size_t np = (size_t)W * H;
    Staging g{c};
    const uint8_t* dref = g.up2d(c->in_a, ref, pitch, W, H);
    // the matched images share one staging buffer
    uint8_t* doth = g.out<uint8_t>(c->in_b, np * (size_t)n);
    const uint8_t* dptr[32];
    for (int i = 0; i < n && g.st == SVA_OK; i++) {
        dptr[i] = doth + (size_t)i * np;
        g.note(hipMemcpy2DAsync(doth + (size_t)i * np, W, others[i], pitch, W, H,
                                hipMemcpyHostToDevice, c->stream),
               "upload");
    }
    uint16_t* dd = g.out<uint16_t>(c->out_a, np * 2);
    float* ds = want_sub ? g.out<float>(c->out_b, np * 4) : nullptr;
    uint16_t* dc = cost_min || cost_second ? g.out<uint16_t>(c->out_c, np * 4) : nullptr;
    if (g.st) return g.st;
    const ConfOut cf{cost_min ? dc : nullptr, cost_second ? dc + np : nullptr, uniqueness,
                     p->invalid};
    const bool conf = cost_min || cost_second || uniqueness;
    if ((s = run_sgm_multi_device(c, dref, dptr, steps, mixed ? red : nullptr, n, W, H, W, p, dd,
                                  ds, conf ? &cf : nullptr)))
        return s;
    g.down(disp, dd, np * 2);
    if (want_sub) g.down(sub, ds, np * 4);
    g.down(cost_min, cf.cost_min, np * 2);
    g.down(cost_second, cf.cost_second, np * 2);
    return g.sync();
}

// The size rules shared by sva_cost_fuse_d, sva_cost_fuse_mixed_d and
// sva_cost_mixed_d: a native-D volume with 32-bit offsets.
int check_stage_volume(Ctx* c, int W, int H, int D, int dreal, int dmin) {
    if (W <= 0 || H <= 0) return fail(c, SVA_ERR_INVALID_ARG, "image size must be positive");
    if (!is_native_d(D))
        return fail(c, SVA_ERR_UNSUPPORTED, "stage entry points take D in {64,128,192,256}");
    if (dreal < 1 || dreal > D) return fail(c, SVA_ERR_INVALID_ARG, "dreal must be 1..D");
    if (dmin < 0 || dmin + D > 65535)
        return fail(c, SVA_ERR_INVALID_ARG, "dmin >= 0 and dmin + D must fit the u16 disparity map");
    if ((unsigned long long)W * (unsigned long long)H * (unsigned)D >= (1ull << 32))
        return fail(c, SVA_ERR_UNSUPPORTED, "W*H*D must be < 2^32 (32-bit volume offsets)");
    return SVA_OK;
}

// sva_cost_fuse_d (ratios null, mixed false) and sva_cost_fuse_mixed_d.
int cost_fuse_d(void* ctx, const uint8_t* volumes, size_t stride, int n, int W, int H, int D,
                int dreal, int dmin, const int32_t* steps, const int32_t* ratios, bool mixed,
                uint8_t* fused) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_steps(c, steps, n))) return s;
    if (!volumes || !fused) return fail(c, SVA_ERR_INVALID_ARG, "null volume");
    if ((s = check_stage_volume(c, W, H, D, dreal, dmin))) return s;
    int32_t red[64];
    if (mixed && (s = check_ratios(c, ratios, n, dmin, dreal, red))) return s;
    // one dwordx4 per lane and volume
    if (((uintptr_t)volumes | (uintptr_t)fused | stride) & 15)
        return fail(c, SVA_ERR_INVALID_ARG, "volumes, stride and fused must be 16-byte aligned");
    if (n > 1 && stride < (size_t)W * H * (size_t)D)
        return fail(c, SVA_ERR_INVALID_ARG, "stride smaller than one volume");
    SVA_HIP(c,
            launch_cost_fuse(*c, volumes, stride, n, W, H, D, dreal, dmin, steps,
                             mixed ? red : nullptr, fused),
            "fuse launch");
    return SVA_OK;
}
}  // namespace

int sva_cost_fuse_d(void* ctx, const uint8_t* volumes, size_t stride, int n, int W, int H, int D,
                    int dreal, int dmin, const int32_t* steps, uint8_t* fused) {
    return cost_fuse_d(ctx, volumes, stride, n, W, H, D, dreal, dmin, steps, nullptr, false, fused);
}

int sva_cost_fuse_mixed_d(void* ctx, const uint8_t* volumes, size_t stride, int n, int W, int H,
                          int D, int dreal, int dmin, const int32_t* steps, const int32_t* ratios,
                          uint8_t* fused) {
    return cost_fuse_d(ctx, volumes, stride, n, W, H, D, dreal, dmin, steps, ratios, true, fused);
}

int sva_cost_mixed_d(void* ctx, const uint64_t* census_ref, const uint64_t* census_oth, int W, int H,
                     int D, int dreal, int dmin, int sx, int sy, int num, int den, uint8_t* C) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    const int32_t step[2] = {sx, sy}, ratio[2] = {num, den};
    int32_t red[2];
    if ((s = check_steps(c, step, 1))) return s;
    if (!census_ref || !census_oth || !C) return fail(c, SVA_ERR_INVALID_ARG, "null buffer");
    if ((s = check_stage_volume(c, W, H, D, dreal, dmin))) return s;
    if ((s = check_ratios(c, ratio, 1, dmin, dreal, red))) return s;
    if (((uintptr_t)census_ref | (uintptr_t)census_oth) & 7 || (uintptr_t)C & 15)
        return fail(c, SVA_ERR_INVALID_ARG, "census maps 8-byte, C 16-byte aligned");
    SVA_HIP(c, launch_cost_mixed(*c, census_ref, census_oth, W, H, D, dmin, sx, sy, red[0], red[1],
                                 C, dreal),
            "cost launch");
    return SVA_OK;
}

int sva_disparity_sgm_multi_d(void* ctx, const uint8_t* ref, const uint8_t* const* others,
                              const int32_t* steps, int n, int W, int H, size_t pitch,
                              const sva_sgm_params* p, int uniqueness, uint16_t* disp, float* sub,
                              uint16_t* cost_min, uint16_t* cost_second) {
    return sgm_multi_d(ctx, ref, others, steps, nullptr, false, n, W, H, pitch, p, uniqueness, disp,
                       sub, cost_min, cost_second);
}

int sva_disparity_sgm_multi(void* ctx, const uint8_t* ref, const uint8_t* const* others,
                            const int32_t* steps, int n, int W, int H, size_t pitch,
                            const sva_sgm_params* p, int uniqueness, uint16_t* disp, float* sub,
                            uint16_t* cost_min, uint16_t* cost_second) {
    return sgm_multi_host(ctx, ref, others, steps, nullptr, false, n, W, H, pitch, p, uniqueness,
                          disp, sub, cost_min, cost_second);
}

int sva_disparity_sgm_mixed_d(void* ctx, const uint8_t* ref, const uint8_t* const* others,
                              const int32_t* steps, const int32_t* ratios, int n, int W, int H,
                              size_t pitch, const sva_sgm_params* p, int uniqueness, uint16_t* disp,
                              float* sub, uint16_t* cost_min, uint16_t* cost_second) {
    return sgm_multi_d(ctx, ref, others, steps, ratios, true, n, W, H, pitch, p, uniqueness, disp,
                       sub, cost_min, cost_second);
}

int sva_disparity_sgm_mixed(void* ctx, const uint8_t* ref, const uint8_t* const* others,
                            const int32_t* steps, const int32_t* ratios, int n, int W, int H,
                            size_t pitch, const sva_sgm_params* p, int uniqueness, uint16_t* disp,
                            float* sub, uint16_t* cost_min, uint16_t* cost_second) {
    return sgm_multi_host(ctx, ref, others, steps, ratios, true, n, W, H, pitch, p, uniqueness, disp,
                          sub, cost_min, cost_second);
}

int sva_disparity_sgm_d(void* ctx, const uint8_t* left, const uint8_t* right, int W, int H,
                        size_t pitch, const sva_sgm_params* p, uint16_t* disp, float* sub) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    if (int s = check_sgm_frame(c, left, right, W, H, pitch, p, 0, disp)) return s;
    return run_sgm_device(c, left, right, W, H, pitch, p, disp, p->subpixel ? sub : nullptr);
}

int sva_disparity_sgm(void* ctx, const uint8_t* left, const uint8_t* right, int W, int H,
                      size_t pitch, const sva_sgm_params* p, uint16_t* disp, float* sub) {
    return sgm_host(ctx, left, right, W, H, pitch, p, false, 0, disp, sub, nullptr, nullptr);
}

int sva_disparity_sgm_conf_d(void* ctx, const uint8_t* left, const uint8_t* right, int W, int H,
                             size_t pitch, const sva_sgm_params* p, int uniqueness, uint16_t* disp,
                             float* sub, uint16_t* cost_min, uint16_t* cost_second) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    if (int s = check_sgm_frame(c, left, right, W, H, pitch, p, uniqueness, disp)) return s;
    const ConfOut cf{cost_min, cost_second, uniqueness, p->invalid};
    return run_sgm_device(c, left, right, W, H, pitch, p, disp, p->subpixel ? sub : nullptr, &cf);
}

int sva_disparity_sgm_conf(void* ctx, const uint8_t* left, const uint8_t* right, int W, int H,
                           size_t pitch, const sva_sgm_params* p, int uniqueness, uint16_t* disp,
                           float* sub, uint16_t* cost_min, uint16_t* cost_second) {
    return sgm_host(ctx, left, right, W, H, pitch, p, true, uniqueness, disp, sub, cost_min,
                    cost_second);
}

int sva_disparity_sgm_batch_d(void* ctx, const sva_pair_d* jobs, int n, int W, int H,
                              size_t pitch, uint16_t* maps, float* sub) {
    return sgm_batch_d(ctx, jobs, n, W, H, pitch, maps, sub, nullptr);
}

// The batch route with the confidence instance: frame j's
// four outputs equal sva_disparity_sgm_conf_d's for that pair.
int sva_disparity_sgm_batch_conf_d(void* ctx, const sva_pair_d* jobs, int n, int W, int H,
                                   size_t pitch, int uniqueness, uint16_t* maps, float* sub,
                                   uint16_t* cost_min, uint16_t* cost_second) {
    const ConfOut cf{cost_min, cost_second, uniqueness,
                     jobs && n > 0 ? jobs[0].params.invalid : 0xffffu};
    return sgm_batch_d(ctx, jobs, n, W, H, pitch, maps, sub, &cf);
}

int sva_census_d(void* ctx, const uint8_t* img, int W, int H, size_t pitch, uint64_t* census) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_image(c, img, W, H, pitch))) return s;
    if (!census) return fail(c, SVA_ERR_INVALID_ARG, "null census output");
    SVA_HIP(c, launch_census(*c, img, W, H, pitch, census), "census launch");
    return SVA_OK;
}

int sva_cost_d(void* ctx, const uint64_t* cl, const uint64_t* cr, int W, int H,
               const sva_sgm_params* p, uint8_t* C) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_sgm(c, p, W, H, true))) return s;
    if (!cl || !cr || !C || W <= 0 || H <= 0) return fail(c, SVA_ERR_INVALID_ARG, "bad argument");
    SVA_HIP(c, launch_cost2(*c, cl, cr, W, H, p->D, p->dmin, p->dir, p->dir_y, C), "cost launch");
    return SVA_OK;
}

int sva_census_cost_d(void* ctx, const uint8_t* left, const uint8_t* right, int W, int H,
                      size_t pitch, const sva_sgm_params* p, uint8_t* C) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_sgm(c, p, W, H, true))) return s;
    if ((s = check_image(c, left, W, H, pitch))) return s;
    if ((s = check_image(c, right, W, H, pitch))) return s;
    if (!C) return fail(c, SVA_ERR_INVALID_ARG, "null cost output");
    const CostRoute route = cost_route(p->D, p->dir, p->dir_y);
    if (route == CostRoute::Split)
        return fail(c, SVA_ERR_UNSUPPORTED,
                    "census+cost kernel: D in {64,128,192,256}, 1-D steps or 2-D steps whose "
                    "primitive form has |dir_y| = 1 and |dir| <= 3");
    SVA_HIP(c, form_cost(*c, route, left, right, W, H, pitch, p->D, p, p->dir, p->dir_y, C, nullptr,
                         nullptr, false),
            "cost launch");
    return SVA_OK;
}

int sva_paths_d(void* ctx, const uint8_t* C, int W, int H, const sva_sgm_params* p, uint8_t* L8) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_sgm(c, p, W, H, true))) return s;
    if (!C || !L8 || W <= 0 || H <= 0) return fail(c, SVA_ERR_INVALID_ARG, "bad argument");
    const AggPlan plan = eight_plan(agg_shape(W, H, p->D, p));
    const AggBuffers b = carve(plan, C, L8, nullptr);
    SVA_HIP(c, launch_paths(*c, plan, b), "paths launch");
    return SVA_OK;
}

int sva_aggregate_d(void* ctx, const uint8_t* C, int W, int H, const sva_sgm_params* p,
                    uint16_t* S) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_sgm(c, p, W, H, true))) return s;
    if (!C || !S || W <= 0 || H <= 0) return fail(c, SVA_ERR_INVALID_ARG, "bad argument");
    const AggPlan plan = eight_plan(agg_shape(W, H, p->D, p));
    SVA_HIP(c, c->paths.ensure(plan.paths_bytes), "path workspace");
    const AggBuffers b = carve(plan, C, c->paths.ptr, nullptr);
    SVA_HIP(c, launch_paths(*c, plan, b), "paths launch");
    SVA_HIP(c, launch_sum(*c, b.volumes, W, H, p->D, S), "sum launch");
    return SVA_OK;
}

int sva_tile_layout_of(int W, int H, int D, sva_tile_layout* out) {
    if (!out || W <= 0 || H <= 0 || !is_native_d(D)) return SVA_ERR_INVALID_ARG;
    *out = tile_layout(W, H, D);
    return SVA_OK;
}

int sva_tile_check(int W, int H, int D, size_t C_bytes, size_t diag_bytes, size_t hckpt_bytes,
                   size_t vckpt_bytes) {
    if (W <= 0 || H <= 0 || !is_native_d(D)) return SVA_ERR_INVALID_ARG;
    const char one = 0;   // any non-null address: sizes only
    return check_tile_buffers(nullptr, W, H, D, &one, C_bytes, &one, diag_bytes, &one, hckpt_bytes,
                              &one, vckpt_bytes);
}

int sva_paths_tile_d(void* ctx, const uint8_t* C, size_t C_bytes, int W, int H,
                     const sva_sgm_params* p, uint8_t* diag, size_t diag_bytes, uint8_t* hckpt,
                     size_t hckpt_bytes, uint8_t* vckpt, size_t vckpt_bytes) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_sgm(c, p, W, H, true))) return s;
    if ((s = check_tile_buffers(c, W, H, p->D, C, C_bytes, diag, diag_bytes, hckpt, hckpt_bytes,
                                vckpt, vckpt_bytes)))
        return s;
    SVA_HIP(c, launch_paths(*c, stage_plan(agg_shape(W, H, p->D, p)),
                            AggBuffers{C, diag, hckpt, vckpt, nullptr}),
            "paths launch");
    return SVA_OK;
}

int sva_wta_hv_d(void* ctx, const uint8_t* C, size_t C_bytes, const uint8_t* diag,
                 size_t diag_bytes, const uint8_t* hckpt, size_t hckpt_bytes, const uint8_t* vckpt,
                 size_t vckpt_bytes, int W, int H, const sva_sgm_params* p, uint16_t* disp,
                 float* sub) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_sgm(c, p, W, H, true))) return s;
    if ((s = check_tile_buffers(c, W, H, p->D, C, C_bytes, diag, diag_bytes, hckpt, hckpt_bytes,
                                vckpt, vckpt_bytes)))
        return s;
    if (!disp) return fail(c, SVA_ERR_INVALID_ARG, "null disparity output");
    // (the kernel only reads the caller's volumes and checkpoints)
    SVA_HIP(c, launch_wta_hv(*c, stage_plan(agg_shape(W, H, p->D, p)),
                             AggBuffers{C, const_cast<uint8_t*>(diag), const_cast<uint8_t*>(hckpt),
                                        const_cast<uint8_t*>(vckpt), nullptr},
                             disp, p->subpixel ? sub : nullptr),
            "wta launch");
    return SVA_OK;
}

int sva_frame_layout_of(int W, int H, const sva_sgm_params* p, long long pair_min_pixels,
                        sva_frame_layout* out) {
    if (!out || W <= 0 || H <= 0 || check_sgm(nullptr, p, W, H) != SVA_OK) return SVA_ERR_INVALID_ARG;
    *out = frame_layout(frame_agg_plan(pair_min_pixels, W, H, padded_D(p->D), p));
    return SVA_OK;
}

int sva_paths_frame_d(void* ctx, const uint8_t* C, size_t C_bytes, int W, int H,
                      const sva_sgm_params* p, uint8_t* volumes, size_t volumes_bytes,
                      uint8_t* ckpt, size_t ckpt_bytes) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_sgm(c, p, W, H))) return s;
    if (W <= 0 || H <= 0) return fail(c, SVA_ERR_INVALID_ARG, "bad argument");
    const AggPlan plan = frame_agg_plan(c->dbg_pair_min_pixels, W, H, padded_D(p->D), p);
    if ((s = check_frame_buffers(c, plan, C, C_bytes, volumes, volumes_bytes, ckpt, ckpt_bytes)))
        return s;
    SVA_HIP(c, launch_paths(*c, plan, carve(plan, C, volumes, ckpt)), "paths launch");
    return SVA_OK;
}

int sva_wta_frame_d(void* ctx, const uint8_t* C, size_t C_bytes, const uint8_t* volumes,
                    size_t volumes_bytes, const uint8_t* ckpt, size_t ckpt_bytes, int W, int H,
                    const sva_sgm_params* p, int uniqueness, uint16_t* disp, float* sub,
                    uint16_t* cost_min, uint16_t* cost_second) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_sgm(c, p, W, H)) || (s = check_uniqueness(c, uniqueness))) return s;
    if (W <= 0 || H <= 0) return fail(c, SVA_ERR_INVALID_ARG, "bad argument");
    const AggPlan plan = frame_agg_plan(c->dbg_pair_min_pixels, W, H, padded_D(p->D), p);
    if ((s = check_frame_buffers(c, plan, C, C_bytes, volumes, volumes_bytes, ckpt, ckpt_bytes)))
        return s;
    if (!disp) return fail(c, SVA_ERR_INVALID_ARG, "null disparity output");
    const ConfOut cf{cost_min, cost_second, uniqueness, p->invalid};
    const bool conf = cost_min || cost_second || uniqueness;
    // (the kernel only reads the caller's volumes and checkpoints)
    SVA_HIP(c, launch_wta_hv(*c, plan, carve(plan, C, const_cast<uint8_t*>(volumes),
                                             const_cast<uint8_t*>(ckpt)),
                             disp, p->subpixel ? sub : nullptr, conf ? &cf : nullptr),
            "wta launch");
    return SVA_OK;
}

int sva_wta_d(void* ctx, const uint16_t* S, int W, int H, const sva_sgm_params* p, uint16_t* disp,
              float* sub) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_sgm(c, p, W, H, true))) return s;
    if (!S || !disp || W <= 0 || H <= 0) return fail(c, SVA_ERR_INVALID_ARG, "bad argument");
    SVA_HIP(c, launch_wta_from_sum(*c, S, W, H, p->D, p->dmin, disp, p->subpixel ? sub : nullptr),
            "wta launch");
    return SVA_OK;
}

int sva_wta_conf_d(void* ctx, const uint16_t* S, int W, int H, const sva_sgm_params* p,
                   int uniqueness, uint16_t* disp, float* sub, uint16_t* cost_min,
                   uint16_t* cost_second) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_sgm(c, p, W, H, true)) || (s = check_uniqueness(c, uniqueness))) return s;
    if (!S || !disp || W <= 0 || H <= 0) return fail(c, SVA_ERR_INVALID_ARG, "bad argument");
    const ConfOut cf{cost_min, cost_second, uniqueness, p->invalid};
    SVA_HIP(c, launch_wta_from_sum(*c, S, W, H, p->D, p->dmin, disp, p->subpixel ? sub : nullptr,
                                   &cf),
            "wta launch");
    return SVA_OK;
}

// ---------------------------------------------------------------- Mode R --
int sva_ref_endpoints_d(void* ctx, int W, int H, const sva_camera* cref, const sva_camera* coth,
                        int k, double t_near, double t_far, int32_t* ends, uint8_t* valid) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_camera(c, cref)) || (s = check_camera(c, coth)) ||
        (s = check_ref_args(c, W, H, k, t_near, t_far)))
        return s;
    if (!ends || !valid) return fail(c, SVA_ERR_INVALID_ARG, "null output");
    SVA_HIP(c, launch_ref_endpoints(*c, W, H, *cref, *coth, k, t_near, t_far, ends, valid),
            "endpoint launch");
    return SVA_OK;
}

namespace {
int check_ref_frame(Ctx* c, const uint8_t* ref, const uint8_t* other, int W, int H, size_t pitch,
                    const sva_camera* cref, const sva_camera* coth, int k, double t_near,
                    double t_far, const uint8_t* d8) {
    int s;
    if ((s = check_image(c, ref, W, H, pitch)) || (s = check_image(c, other, W, H, pitch)) ||
        (s = check_camera(c, cref)) || (s = check_camera(c, coth)) ||
        (s = check_ref_args(c, W, H, k, t_near, t_far)))
        return s;
    if (!d8) return fail(c, SVA_ERR_INVALID_ARG, "null disparity output");
    return SVA_OK;
}
}  // namespace

int sva_disparity_ref_d(void* ctx, const uint8_t* ref, const uint8_t* other, int W, int H,
                        size_t pitch, const uint8_t* mask, const sva_camera* cref,
                        const sva_camera* coth, int k, double t_near, double t_far, uint8_t* d8,
                        uint16_t* d16, uint8_t* valid) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    if (int s = check_ref_frame(c, ref, other, W, H, pitch, cref, coth, k, t_near, t_far, d8))
        return s;
    return run_ref_device(c, ref, other, W, H, pitch, mask, cref, coth, k, t_near, t_far, d8, d16,
                          valid);
}

int sva_disparity_ref(void* ctx, const uint8_t* ref, const uint8_t* other, int W, int H,
                      size_t pitch, const uint8_t* mask, const sva_camera* cref,
                      const sva_camera* coth, int k, double t_near, double t_far, uint8_t* d8,
                      uint16_t* d16, uint8_t* valid) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_ref_frame(c, ref, other, W, H, pitch, cref, coth, k, t_near, t_far, d8)))
        return s;
    const size_t np = (size_t)W * H;
    Staging g{c};
    const uint8_t* dref = g.up2d(c->in_a, ref, pitch, W, H);
    const uint8_t* doth = g.up2d(c->in_b, other, pitch, W, H);
    const uint8_t* dmask = mask ? g.up<uint8_t>(c->in_mask, mask, np) : nullptr;
    // untouched pixels keep the caller's values (CameraStereoVision.cpp:46,55)
    uint8_t* o8 = g.up<uint8_t>(c->out_a, d8, np);
    uint16_t* o16 = d16 ? g.up<uint16_t>(c->out_b, d16, np * 2) : nullptr;
    uint8_t* ov = valid ? g.up<uint8_t>(c->out_c, valid, np) : nullptr;
    if (g.st) return g.st;
    if ((s = run_ref_device(c, dref, doth, W, H, W, dmask, cref, coth, k, t_near, t_far, o8, o16,
                            ov)))
        return s;
    g.down(d8, o8, np);
    g.down(d16, o16, np * 2);
    g.down(valid, ov, np);
    return g.sync();
}

int sva_disparity_to_depth_d(void* ctx, const uint8_t* disp, int n, double cam_distance,
                             double f, double pixel_size, double* depth) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    if (!disp || !depth || n < 0) return fail(c, SVA_ERR_INVALID_ARG, "bad argument");
    if (n == 0) return SVA_OK;
    SVA_HIP(c, launch_disp_to_depth(*c, disp, n, cam_distance, f, pixel_size, depth), "depth launch");
    return SVA_OK;
}

int sva_disparity_to_depth(void* ctx, const uint8_t* disp, int n, double cam_distance, double f,
                           double pixel_size, double* depth) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    if (!disp || !depth || n < 0) return fail(c, SVA_ERR_INVALID_ARG, "bad argument");
    if (n == 0) return SVA_OK;
    Staging g{c};
    const uint8_t* dd = g.up<uint8_t>(c->in_a, disp, (size_t)n);
    double* dz = g.out<double>(c->out_a, (size_t)n * 8);
    if (g.st) return g.st;
    SVA_HIP(c, launch_disp_to_depth(*c, dd, n, cam_distance, f, pixel_size, dz), "depth launch");
    g.down(depth, dz, (size_t)n * 8);
    return g.sync();
}

namespace {
// One fusion call: the planes are all on the host
// or all on the device.  subpix: the sub-pixel forms; cost_min, cost_second and
// winner: the cost-aware ones.
struct FuseArgs {
    const uint16_t* disps;
    const float* subpix;
    const uint16_t *cost_min, *cost_second;
    int n_maps, W, H;
    const double* baselines;
    double f, pixel_size;
    uint16_t invalid;
    int mode;   // SVA_FUSE_MEDIAN from the median entries
    double* depth;
    uint8_t *n_valid, *winner;
};

// The rules of the eight entries, in sva.h's order.  by_cost: a cost-aware entry,
// which takes its mode from the caller and refuses SVA_FUSE_MEDIAN; sub: a
// sub-pixel entry, whose own rule comes after those of its u16 form.
int check_fuse(Ctx* c, const FuseArgs& a, bool by_cost, bool sub) {
    if (!a.disps || (by_cost && !a.cost_min) || !a.baselines || !a.depth)
        return fail(c, SVA_ERR_INVALID_ARG, "null pointer");
    if (by_cost && a.mode != SVA_FUSE_MIN_COST && a.mode != SVA_FUSE_MAX_MARGIN)
        return fail(c, SVA_ERR_INVALID_ARG, "mode must be SVA_FUSE_MIN_COST or SVA_FUSE_MAX_MARGIN");
    if (by_cost && a.mode == SVA_FUSE_MAX_MARGIN && !a.cost_second)
        return fail(c, SVA_ERR_INVALID_ARG, "SVA_FUSE_MAX_MARGIN needs the cost_second planes");
    if (a.n_maps < 1 || a.n_maps > 32)
        return fail(c, by_cost ? SVA_ERR_INVALID_ARG : SVA_ERR_UNSUPPORTED, "n_maps must be 1..32");
    if (a.W <= 0 || a.H <= 0) return fail(c, SVA_ERR_INVALID_ARG, "image size must be positive");
    if (sub && !a.subpix) return fail(c, SVA_ERR_INVALID_ARG, "null subpix");
    return SVA_OK;
}

// A checked call on device planes.
int run_fuse(Ctx* c, const FuseArgs& a) {
    double num[32];
    for (int i = 0; i < a.n_maps; i++) num[i] = a.baselines[i] * a.f;
    SVA_HIP(c,
            launch_fuse(*c, a.disps, a.subpix, a.cost_min, a.cost_second, a.n_maps,
                        (size_t)a.W * a.H, num, a.pixel_size, a.invalid, a.mode, a.depth, a.n_valid,
                        a.winner),
            "fuse launch");
    return SVA_OK;
}

// A checked call on host planes.  The f32 planes of the sub-pixel forms stage
// through in_mask, the fourth input buffer.
int fuse_host(Ctx* c, const FuseArgs& a) {
    const size_t np = (size_t)a.W * a.H, in_bytes = np * 2 * (size_t)a.n_maps;
    Staging g{c};
    FuseArgs d = a;
    d.disps = g.up<uint16_t>(c->in_a, a.disps, in_bytes);
    if (a.subpix) d.subpix = g.up<float>(c->in_mask, a.subpix, in_bytes * 2);
    if (a.cost_min) d.cost_min = g.up<uint16_t>(c->in_b, a.cost_min, in_bytes);
    if (a.cost_second) d.cost_second = g.up<uint16_t>(c->in_c, a.cost_second, in_bytes);
    d.depth = g.out<double>(c->out_a, np * 8);
    d.n_valid = g.out<uint8_t>(c->out_b, np);
    d.winner = a.mode == SVA_FUSE_MEDIAN ? nullptr : g.out<uint8_t>(c->out_c, np);
    if (g.st) return g.st;
    if (int s = run_fuse(c, d)) return s;
    g.down(a.depth, d.depth, np * 8);
    g.down(a.n_valid, d.n_valid, np);
    g.down(a.winner, d.winner, np);
    return g.sync();
}

// What tells the eight entries apart: a cost-aware one, a sub-pixel one, host planes.
enum : unsigned { kFuseByCost = 1, kFuseSub = 2, kFuseHost = 4 };

int fuse_entry(void* ctx, const FuseArgs& a, unsigned kind) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    if (int s = check_fuse(c, a, kind & kFuseByCost, kind & kFuseSub)) return s;
    return (kind & kFuseHost) ? fuse_host(c, a) : run_fuse(c, a);
}
}  // namespace

int sva_fuse_depth_d(void* ctx, const uint16_t* disps, int n_maps, int W, int H,
                     const double* baselines, double f, double pixel_size, uint16_t invalid,
                     double* depth, uint8_t* n_valid) {
    return fuse_entry(ctx, {disps, nullptr, nullptr, nullptr, n_maps, W, H, baselines, f, pixel_size,
                            invalid, SVA_FUSE_MEDIAN, depth, n_valid, nullptr},
                      0);
}

int sva_fuse_depth(void* ctx, const uint16_t* disps, int n_maps, int W, int H,
                   const double* baselines, double f, double pixel_size, uint16_t invalid,
                   double* depth, uint8_t* n_valid) {
    return fuse_entry(ctx, {disps, nullptr, nullptr, nullptr, n_maps, W, H, baselines, f, pixel_size,
                            invalid, SVA_FUSE_MEDIAN, depth, n_valid, nullptr},
                      kFuseHost);
}

int sva_fuse_depth_conf_d(void* ctx, const uint16_t* disps, const uint16_t* cost_min,
                          const uint16_t* cost_second, int n_maps, int W, int H,
                          const double* baselines, double f, double pixel_size, uint16_t invalid,
                          int mode, double* depth, uint8_t* n_valid, uint8_t* winner) {
    return fuse_entry(ctx, {disps, nullptr, cost_min, cost_second, n_maps, W, H, baselines, f,
                            pixel_size, invalid, mode, depth, n_valid, winner},
                      kFuseByCost);
}

int sva_fuse_depth_conf(void* ctx, const uint16_t* disps, const uint16_t* cost_min,
                        const uint16_t* cost_second, int n_maps, int W, int H,
                        const double* baselines, double f, double pixel_size, uint16_t invalid,
                        int mode, double* depth, uint8_t* n_valid, uint8_t* winner) {
    return fuse_entry(ctx, {disps, nullptr, cost_min, cost_second, n_maps, W, H, baselines, f,
                            pixel_size, invalid, mode, depth, n_valid, winner},
                      kFuseByCost | kFuseHost);
}

// Sub-pixel fusion: the four calls above on the f32 maps.
int sva_fuse_depth_sub_d(void* ctx, const uint16_t* disps, const float* subpix, int n_maps, int W,
                         int H, const double* baselines, double f, double pixel_size,
                         uint16_t invalid, double* depth, uint8_t* n_valid) {
    return fuse_entry(ctx, {disps, subpix, nullptr, nullptr, n_maps, W, H, baselines, f, pixel_size,
                            invalid, SVA_FUSE_MEDIAN, depth, n_valid, nullptr},
                      kFuseSub);
}

int sva_fuse_depth_sub(void* ctx, const uint16_t* disps, const float* subpix, int n_maps, int W,
                       int H, const double* baselines, double f, double pixel_size,
                       uint16_t invalid, double* depth, uint8_t* n_valid) {
    return fuse_entry(ctx, {disps, subpix, nullptr, nullptr, n_maps, W, H, baselines, f, pixel_size,
                            invalid, SVA_FUSE_MEDIAN, depth, n_valid, nullptr},
                      kFuseSub | kFuseHost);
}

int sva_fuse_depth_conf_sub_d(void* ctx, const uint16_t* disps, const float* subpix,
                              const uint16_t* cost_min, const uint16_t* cost_second, int n_maps,
                              int W, int H, const double* baselines, double f, double pixel_size,
                              uint16_t invalid, int mode, double* depth, uint8_t* n_valid,
                              uint8_t* winner) {
    return fuse_entry(ctx, {disps, subpix, cost_min, cost_second, n_maps, W, H, baselines, f,
                            pixel_size, invalid, mode, depth, n_valid, winner},
                      kFuseByCost | kFuseSub);
}

int sva_fuse_depth_conf_sub(void* ctx, const uint16_t* disps, const float* subpix,
                            const uint16_t* cost_min, const uint16_t* cost_second, int n_maps,
                            int W, int H, const double* baselines, double f, double pixel_size,
                            uint16_t invalid, int mode, double* depth, uint8_t* n_valid,
                            uint8_t* winner) {
    return fuse_entry(ctx, {disps, subpix, cost_min, cost_second, n_maps, W, H, baselines, f,
                            pixel_size, invalid, mode, depth, n_valid, winner},
                      kFuseByCost | kFuseSub | kFuseHost);
}

// ----------------- the map filters of the post-filter chain --
// sva_cross_check, sva_filter_speckles, sva_fill_holes, sva_weighted_median and
// their _d twins.  Each builds its args struct (map_filter_args.h, which also
// has check_x, the rules) from the positional ABI and goes through filter_entry
// (above, with run_x and the host staging).
int sva_cross_check_d(void* ctx, const uint16_t* disps, const float* subpix, int n, int W, int H,
                      const int32_t* view_step, uint16_t invalid, int max_diff, int min_agree,
                      int max_conflict, uint16_t* out, float* out_sub, uint8_t* agree,
                      uint8_t* conflict) {
    return filter_entry<CrossArgs>(ctx, {{disps, subpix, n, W, H, invalid, out, out_sub}, view_step,
                                         max_diff, min_agree, max_conflict, agree, conflict},
                                   check_cross, run_cross, nullptr);
}

int sva_cross_check(void* ctx, const uint16_t* disps, const float* subpix, int n, int W, int H,
                    const int32_t* view_step, uint16_t invalid, int max_diff, int min_agree,
                    int max_conflict, uint16_t* out, float* out_sub, uint8_t* agree,
                    uint8_t* conflict) {
    return filter_entry<CrossArgs>(ctx, {{disps, subpix, n, W, H, invalid, out, out_sub}, view_step,
                                         max_diff, min_agree, max_conflict, agree, conflict},
                                   check_cross, run_cross, cross_host);
}

int sva_filter_speckles_d(void* ctx, const uint16_t* disps, const float* subpix, int n, int W,
                          int H, uint16_t invalid, int max_size, int max_diff, uint16_t* out,
                          float* out_sub, uint32_t* comp_size) {
    return filter_entry<SpeckleArgs>(ctx, {{disps, subpix, n, W, H, invalid, out, out_sub}, max_size,
                                           max_diff, comp_size},
                                     check_speckle, run_speckle, nullptr);
}

int sva_filter_speckles(void* ctx, const uint16_t* disps, const float* subpix, int n, int W, int H,
                        uint16_t invalid, int max_size, int max_diff, uint16_t* out, float* out_sub,
                        uint32_t* comp_size) {
    return filter_entry<SpeckleArgs>(ctx, {{disps, subpix, n, W, H, invalid, out, out_sub}, max_size,
                                           max_diff, comp_size},
                                     check_speckle, run_speckle, speckle_host);
}

int sva_fill_holes_d(void* ctx, const uint16_t* disps, const float* subpix, int n, int W, int H,
                     uint16_t invalid, int max_dist, int min_found, int mode, uint16_t* out,
                     float* out_sub, uint8_t* n_found) {
    return filter_entry<FillArgs>(ctx, {{disps, subpix, n, W, H, invalid, out, out_sub}, max_dist,
                                        min_found, mode, n_found},
                                  check_fill, run_fill, nullptr);
}

int sva_fill_holes(void* ctx, const uint16_t* disps, const float* subpix, int n, int W, int H,
                   uint16_t invalid, int max_dist, int min_found, int mode, uint16_t* out,
                   float* out_sub, uint8_t* n_found) {
    return filter_entry<FillArgs>(ctx, {{disps, subpix, n, W, H, invalid, out, out_sub}, max_dist,
                                        min_found, mode, n_found},
                                  check_fill, run_fill, fill_host);
}

int sva_weighted_median_d(void* ctx, const uint16_t* disps, const float* subpix,
                          const uint8_t* const* guides, size_t guide_pitch,
                          const uint16_t* weights, const uint8_t* select, int n, int W, int H,
                          uint16_t invalid, int radius, int min_support, int fill, uint16_t* out,
                          float* out_sub, uint16_t* support) {
    return filter_entry<WmedArgs>(ctx, {{disps, subpix, n, W, H, invalid, out, out_sub}, guides,
                                        guide_pitch, weights, select, radius, min_support, fill,
                                        support},
                                  check_wmed, run_wmed, nullptr);
}

int sva_weighted_median(void* ctx, const uint16_t* disps, const float* subpix,
                        const uint8_t* const* guides, size_t guide_pitch, const uint16_t* weights,
                        const uint8_t* select, int n, int W, int H, uint16_t invalid, int radius,
                        int min_support, int fill, uint16_t* out, float* out_sub,
                        uint16_t* support) {
    return filter_entry<WmedArgs>(ctx, {{disps, subpix, n, W, H, invalid, out, out_sub}, guides,
                                        guide_pitch, weights, select, radius, min_support, fill,
                                        support},
                                  check_wmed, run_wmed, wmed_host);
}

// ------------------------- rectification and masking --
int sva_rectify_d(void* ctx, const uint8_t* src, int n, int src_w, int src_h, size_t src_pitch,
                  const sva_rectify_view* views, int out_w, int out_h, size_t out_pitch,
                  int border, uint8_t* out, uint8_t* valid, int32_t* map) {
    return filter_entry<RectifyArgs>(ctx, {src, n, src_w, src_h, src_pitch, views, out_w, out_h,
                                           out_pitch, border, out, valid, map},
                                     check_rectify, run_rectify, nullptr);
}

int sva_rectify(void* ctx, const uint8_t* src, int n, int src_w, int src_h, size_t src_pitch,
                const sva_rectify_view* views, int out_w, int out_h, size_t out_pitch, int border,
                uint8_t* out, uint8_t* valid, int32_t* map) {
    return filter_entry<RectifyArgs>(ctx, {src, n, src_w, src_h, src_pitch, views, out_w, out_h,
                                           out_pitch, border, out, valid, map},
                                     check_rectify, run_rectify, rectify_host);
}

int sva_rectify_view_of(const double K_raw[9], const double dist[5], const double R[9],
                        const double K_ideal[9], sva_rectify_view* out) {
    return rc::view_of(K_raw, dist, R, K_ideal, out) ? SVA_ERR_INVALID_ARG : SVA_OK;
}

int sva_mask_maps_d(void* ctx, const uint16_t* disps, const float* subpix, int n, int W, int H,
                    const uint8_t* valid, uint16_t invalid, uint16_t* out, float* out_sub) {
    return filter_entry<MaskArgs>(ctx, {{disps, subpix, n, W, H, invalid, out, out_sub}, valid},
                                  check_mask, run_mask, nullptr);
}

int sva_mask_maps(void* ctx, const uint16_t* disps, const float* subpix, int n, int W, int H,
                  const uint8_t* valid, uint16_t invalid, uint16_t* out, float* out_sub) {
    return filter_entry<MaskArgs>(ctx, {{disps, subpix, n, W, H, invalid, out, out_sub}, valid},
                                  check_mask, run_mask, mask_host);
}

// ------------------------------------------ refinement / 3-D --
namespace {
int check_shift(Ctx* c, const sva_camera* in_cam, const sva_camera* out_cam, const void* a,
                const void* b, const void* out, int W, int H, size_t pitch) {
    int s;
    if ((s = check_planes(c, W, H, pitch)) || (s = check_camera(c, in_cam)) ||
        (s = check_camera(c, out_cam)))
        return s;
    if (!a || !b || !out) return fail(c, SVA_ERR_INVALID_ARG, "null plane");
    return SVA_OK;
}

int check_improve(Ctx* c, const uint8_t* disparity, const uint8_t* center,
                  const uint8_t* const* images, const sva_camera* cam_pairs, int n_pairs, int W,
                  int H, size_t pitch, int window_size, const uint8_t* out) {
    int s;
    if ((s = check_planes(c, W, H, pitch)) || (s = check_window(c, window_size))) return s;
    if (n_pairs < 0 || (n_pairs > 0 && (!images || !cam_pairs)))
        return fail(c, SVA_ERR_INVALID_ARG, "bad pair list");
    if (!disparity || !center || !out) return fail(c, SVA_ERR_INVALID_ARG, "null plane");
    for (int i = 0; i < n_pairs; i++)
        if (!images[i]) return fail(c, SVA_ERR_INVALID_ARG, "null pair image");
    return SVA_OK;
}

int run_shift2(Ctx* c, const sva_camera* in_cam, const sva_camera* out_cam, const double* depth,
               int W, int H, double* shifted) {
    SVA_HIP(c, c->keys.ensure((size_t)W * H * 4), "key workspace");
    SVA_HIP(c, launch_shift_perspective2(*c, *in_cam, *out_cam, depth, W, H,
                                         (unsigned*)c->keys.ptr, shifted), "shift2 launch");
    return SVA_OK;
}

int check_points_to_depth(Ctx* c, const double* points, int64_t n_points, const sva_camera* cam,
                          int W, int H, const double* depth) {
    int s;
    if ((s = check_planes(c, W, H, (size_t)W)) || (s = check_camera(c, cam))) return s;
    if (n_points < 0 || n_points > 0xfffffffell || (n_points > 0 && !points) || !depth)
        return fail(c, SVA_ERR_INVALID_ARG, "bad point list");
    return SVA_OK;
}

int run_points_to_depth(Ctx* c, const double* points, int64_t n_points, const sva_camera* cam,
                        int W, int H, double* depth) {
    SVA_HIP(c, c->keys.ensure((size_t)W * H * 4), "key workspace");
    SVA_HIP(c, launch_points_to_depth(*c, points, n_points, *cam, W, H, (unsigned*)c->keys.ptr,
                                      depth), "points launch");
    return SVA_OK;
}

int check_depth_to_points(Ctx* c, const double* depth, int W, int H, const sva_camera* cam,
                          const double* points, const int64_t* n_points) {
    int s;
    if ((s = check_planes(c, W, H, (size_t)W)) || (s = check_camera(c, cam))) return s;
    if (!depth || !points || !n_points) return fail(c, SVA_ERR_INVALID_ARG, "null argument");
    return SVA_OK;
}

// The points of a device depth map, compacted into device `points`; *n (host)
// is their number once this returns (it synchronises).
int run_depth_to_points(Ctx* c, const double* depth, int W, int H, const sva_camera* cam,
                        double* points, long long* n) {
    SVA_HIP(c, c->counts.ensure(d2p_units(W, H) * 4), "count workspace");
    SVA_HIP(c, c->total.ensure(sizeof(long long)), "count workspace");
    SVA_HIP(c, launch_depth_to_points(*c, depth, W, H, *cam, (unsigned*)c->counts.ptr,
                                      (long long*)c->total.ptr, points), "d2p launch");
    SVA_HIP(c, hipMemcpyAsync(n, c->total.ptr, sizeof(*n), hipMemcpyDeviceToHost, c->stream),
            "download");
    SVA_HIP(c, hipStreamSynchronize(c->stream), "sync");
    return SVA_OK;
}
}  // namespace

int sva_shift_perspective_d(void* ctx, const sva_camera* in_cam, const sva_camera* out_cam,
                            const uint8_t* disparity, const uint8_t* image, int W, int H,
                            size_t pitch, uint8_t* shifted) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    if (int s = check_shift(c, in_cam, out_cam, disparity, image, shifted, W, H, pitch)) return s;
    SVA_HIP(c, launch_shift_perspective(*c, *in_cam, *out_cam, disparity, image, W, H, pitch,
                                        shifted), "shift launch");
    return SVA_OK;
}

int sva_shift_perspective(void* ctx, const sva_camera* in_cam, const sva_camera* out_cam,
                          const uint8_t* disparity, const uint8_t* image, int W, int H,
                          size_t pitch, uint8_t* shifted) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    if (int s = check_shift(c, in_cam, out_cam, disparity, image, shifted, W, H, pitch)) return s;
    const size_t bytes = (size_t)H * pitch;
    Staging g{c};
    const uint8_t* dd = g.up<uint8_t>(c->in_a, disparity, bytes);
    const uint8_t* di = g.up<uint8_t>(c->in_b, image, bytes);
    // pixels no source pixel lands on keep the caller's values
    uint8_t* ds = g.up<uint8_t>(c->out_a, shifted, bytes);
    if (g.st) return g.st;
    SVA_HIP(c, launch_shift_perspective(*c, *in_cam, *out_cam, dd, di, W, H, pitch, ds),
            "shift launch");
    g.down(shifted, ds, bytes);
    return g.sync();
}

int sva_improve_with_disparity_d(void* ctx, const uint8_t* disparity, const uint8_t* center,
                                 const uint8_t* const* images, const sva_camera* cam_pairs,
                                 int n_pairs, int W, int H, size_t pitch, const uint8_t* mask,
                                 int window_size, int strict, uint8_t* out) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    if (int s = check_improve(c, disparity, center, images, cam_pairs, n_pairs, W, H, pitch,
                              window_size, out))
        return s;
    return run_improve(c, disparity, center, images, cam_pairs, n_pairs, W, H, pitch, mask,
                       window_size, strict, out, nullptr);
}

int sva_improve_with_disparity(void* ctx, const uint8_t* disparity, const uint8_t* center,
                               const uint8_t* const* images, const sva_camera* cam_pairs,
                               int n_pairs, int W, int H, size_t pitch, const uint8_t* mask,
                               int window_size, int strict, uint8_t* out) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_improve(c, disparity, center, images, cam_pairs, n_pairs, W, H, pitch,
                           window_size, out)))
        return s;
    const size_t bytes = (size_t)H * pitch;
    Staging g{c};
    const uint8_t* dd = g.up<uint8_t>(c->in_a, disparity, bytes);
    const uint8_t* dc = g.up<uint8_t>(c->in_b, center, bytes);
    const uint8_t* dmask = mask ? g.up<uint8_t>(c->in_mask, mask, bytes) : nullptr;
    // pixels the refinement does not reach keep the caller's values
    uint8_t* dout = g.up<uint8_t>(c->out_a, out, bytes);
    uint8_t* dimg = g.out<uint8_t>(c->in_c, bytes);
    if (g.st) return g.st;
    auto fetch = [&](int i, const uint8_t** img) -> int {
        // one staging buffer reused per pair: stream order keeps the upload
        // of pair i behind pair i-1's kernels
        SVA_HIP(c, hipMemcpyAsync(dimg, images[i], bytes, hipMemcpyHostToDevice, c->stream),
                "upload");
        *img = dimg;
        return SVA_OK;
    };
    if ((s = run_improve(c, dd, dc, nullptr, cam_pairs, n_pairs, W, H, pitch, dmask, window_size,
                         strict, dout, fetch)))
        return s;
    g.down(out, dout, bytes);
    return g.sync();
}

int sva_shift_perspective2_d(void* ctx, const sva_camera* in_cam, const sva_camera* out_cam,
                             const double* depth, int W, int H, double* shifted) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    if (int s = check_shift(c, in_cam, out_cam, depth, depth, shifted, W, H, (size_t)W)) return s;
    return run_shift2(c, in_cam, out_cam, depth, W, H, shifted);
}

int sva_shift_perspective2(void* ctx, const sva_camera* in_cam, const sva_camera* out_cam,
                           const double* depth, int W, int H, double* shifted) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_shift(c, in_cam, out_cam, depth, depth, shifted, W, H, (size_t)W))) return s;
    const size_t bytes = (size_t)W * H * 8;
    Staging g{c};
    const double* dd = g.up<double>(c->in_a, depth, bytes);
    double* ds = g.up<double>(c->out_a, shifted, bytes);   // (untouched pixels: the caller's)
    if (g.st) return g.st;
    if ((s = run_shift2(c, in_cam, out_cam, dd, W, H, ds))) return s;
    g.down(shifted, ds, bytes);
    return g.sync();
}

int sva_points_to_depth_d(void* ctx, const double* points, int64_t n_points,
                          const sva_camera* cam, int W, int H, double* depth) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    if (int s = check_points_to_depth(c, points, n_points, cam, W, H, depth)) return s;
    return run_points_to_depth(c, points, n_points, cam, W, H, depth);
}

int sva_points_to_depth(void* ctx, const double* points, int64_t n_points, const sva_camera* cam,
                        int W, int H, double* depth) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_points_to_depth(c, points, n_points, cam, W, H, depth))) return s;
    const size_t pbytes = (size_t)n_points * 24, dbytes = (size_t)W * H * 8;
    Staging g{c};
    const double* dp = pbytes ? g.up<double>(c->in_a, points, pbytes) : g.out<double>(c->in_a, 8);
    double* dz = g.up<double>(c->out_a, depth, dbytes);     // (untouched pixels: the caller's)
    if (g.st) return g.st;
    if ((s = run_points_to_depth(c, dp, n_points, cam, W, H, dz))) return s;
    g.down(depth, dz, dbytes);
    return g.sync();
}

int sva_depth_to_points_d(void* ctx, const double* depth, int W, int H, const sva_camera* cam,
                          double* points, int64_t* n_points) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_depth_to_points(c, depth, W, H, cam, points, n_points))) return s;
    long long n = 0;
    if ((s = run_depth_to_points(c, depth, W, H, cam, points, &n))) return s;
    *n_points = n;
    return SVA_OK;
}

int sva_depth_to_points(void* ctx, const double* depth, int W, int H, const sva_camera* cam,
                        double* points, int64_t* n_points) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_depth_to_points(c, depth, W, H, cam, points, n_points))) return s;
    const size_t np = (size_t)W * H;
    Staging g{c};
    const double* dd = g.up<double>(c->in_a, depth, np * 8);
    double* dp = g.out<double>(c->out_a, np * 24);
    if (g.st) return g.st;
    long long n = 0;
    if ((s = run_depth_to_points(c, dd, W, H, cam, dp, &n))) return s;
    // (n is known only after that synchronise: the n points, then a second one)
    if (n > 0) g.down(points, dp, (size_t)n * 24);
    if ((s = g.sync())) return s;
    *n_points = n;
    return SVA_OK;
}

// ---------------------------------------------------- ingestion (§8f 4) --
int sva_resize_half_size(int W, int H, int* out_w, int* out_h) {
    if (W < 0 || H < 0 || !out_w || !out_h) return SVA_ERR_INVALID_ARG;
    resize_half_size(W, H, out_w, out_h);
    return SVA_OK;
}

namespace {
// *dst_rows: the output's rows, 0 when it has no pixels.
int check_resize_half(Ctx* c, const uint8_t* src, int W, int H, size_t pitch, const uint8_t* dst,
                      size_t dst_pitch, size_t* dst_rows) {
    int s, dw, dh;
    if ((s = check_planes(c, W, H, pitch))) return s;
    resize_half_size(W, H, &dw, &dh);
    if (!src || (!dst && dw > 0 && dh > 0) || dst_pitch < (size_t)dw)
        return fail(c, SVA_ERR_INVALID_ARG, "bad resize argument");
    *dst_rows = dw > 0 ? (size_t)dh : 0;
    return SVA_OK;
}
}  // namespace

int sva_resize_half_d(void* ctx, const uint8_t* src, int W, int H, size_t pitch, uint8_t* dst,
                      size_t dst_pitch) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    size_t rows;
    if (int s = check_resize_half(c, src, W, H, pitch, dst, dst_pitch, &rows)) return s;
    SVA_HIP(c, launch_resize_half(*c, src, W, H, pitch, dst, dst_pitch), "resize launch");
    return SVA_OK;
}

int sva_resize_half(void* ctx, const uint8_t* src, int W, int H, size_t pitch, uint8_t* dst,
                    size_t dst_pitch) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    size_t rows;
    if (int s = check_resize_half(c, src, W, H, pitch, dst, dst_pitch, &rows)) return s;
    if (rows == 0) return SVA_OK;    // an empty output (the host form only)
    const size_t db = rows * dst_pitch;
    Staging g{c};
    const uint8_t* ds = g.up<uint8_t>(c->in_a, src, (size_t)H * pitch);
    uint8_t* dd = g.out<uint8_t>(c->out_a, db);
    if (g.st) return g.st;
    SVA_HIP(c, launch_resize_half(*c, ds, W, H, pitch, dd, dst_pitch), "resize launch");
    // only the pixels go back: the bytes between the caller's rows are not touched
    int dw, dh;
    resize_half_size(W, H, &dw, &dh);
    g.note(hipMemcpy2DAsync(dst, dst_pitch, dd, dst_pitch, (size_t)dw, (size_t)dh,
                            hipMemcpyDeviceToHost, c->stream), "download");
    return g.sync();
}

// ----------------------------------------------------------- evaluation --
namespace {
int check_dims(Ctx* c, int w, int h) {
    if (w <= 0 || h <= 0 || (size_t)w * h > ((size_t)1 << 31))
        return fail(c, SVA_ERR_INVALID_ARG, "matrix dimensions must be positive (< 2^31 elements)");
    return SVA_OK;
}

// sva_resize_linear_f64[_d] (ref unused) and sva_ref_error[_d] (need_ref):
// dst = resize(src, dw x dh), with ref (dst - ref) * scale.  host: the
// buffers are the caller's host memory.
int resize_entry(void* ctx, bool host, const double* src, int sw, int sh, const double* ref,
                 bool need_ref, int dw, int dh, double scale, double* dst) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    int s;
    if ((s = check_dims(c, sw, sh)) || (s = check_dims(c, dw, dh))) return s;
    if (!src || !dst || (need_ref && !ref)) return fail(c, SVA_ERR_INVALID_ARG, "null matrix");
    Staging g{c};
    double* out = dst;
    if (host) {
        const size_t db = (size_t)dw * dh * 8;
        src = g.up<double>(c->in_a, src, (size_t)sw * sh * 8);
        out = g.out<double>(c->out_a, db);
        if (ref) ref = g.up<double>(c->in_b, ref, db);
        if (g.st) return g.st;
    }
    SVA_HIP(c, launch_resize_linear(*c, src, sw, sh, out, dw, dh, ref, scale), "resize launch");
    if (!host) return SVA_OK;
    g.down(dst, out, (size_t)dw * dh * 8);
    return g.sync();
}

int check_mean(Ctx* c, const double* image, int w, int h, const double* mean) {
    if (int s = check_dims(c, w, h)) return s;
    if (!image || !mean) return fail(c, SVA_ERR_INVALID_ARG, "null argument");
    return SVA_OK;
}

// cv::mean(image, mask)[0] of device buffers into host *mean (synchronises).
int run_mean(Ctx* c, const double* image, const uint8_t* mask, size_t n, double* mean) {
    SVA_HIP(c, c->scratch_u16.ensure(masked_mean_workspace()), "reduction workspace");
    double* dmean = (double*)((char*)c->scratch_u16.ptr + masked_mean_workspace() - sizeof(double));
    SVA_HIP(c, launch_masked_mean(*c, image, mask, n, c->scratch_u16.ptr, dmean), "mean launch");
    SVA_HIP(c, hipMemcpyAsync(mean, dmean, sizeof(double), hipMemcpyDeviceToHost, c->stream),
            "download");
    SVA_HIP(c, hipStreamSynchronize(c->stream), "sync");
    return SVA_OK;
}
}  // namespace

int sva_resize_linear_f64_d(void* ctx, const double* src, int sw, int sh, double* dst, int dw,
                            int dh) {
    return resize_entry(ctx, false, src, sw, sh, nullptr, false, dw, dh, 0.0, dst);
}

int sva_resize_linear_f64(void* ctx, const double* src, int sw, int sh, double* dst, int dw,
                          int dh) {
    return resize_entry(ctx, true, src, sw, sh, nullptr, false, dw, dh, 0.0, dst);
}

int sva_ref_error_d(void* ctx, const double* depth, int w, int h, const double* ref, int rw,
                    int rh, double scale, double* error) {
    return resize_entry(ctx, false, depth, w, h, ref, true, rw, rh, scale, error);
}

int sva_ref_error(void* ctx, const double* depth, int w, int h, const double* ref, int rw, int rh,
                  double scale, double* error) {
    return resize_entry(ctx, true, depth, w, h, ref, true, rw, rh, scale, error);
}

int sva_masked_mean_d(void* ctx, const double* image, const uint8_t* mask, int w, int h,
                      double* mean) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    if (int s = check_mean(c, image, w, h, mean)) return s;
    return run_mean(c, image, mask, (size_t)w * h, mean);
}

int sva_masked_mean(void* ctx, const double* image, const uint8_t* mask, int w, int h,
                    double* mean) {
    Ctx* c = as_ctx(ctx);
    SVA_CHECK_CTX(c);
    if (int s = check_mean(c, image, w, h, mean)) return s;
    const size_t n = (size_t)w * h;
    Staging g{c};
    const double* di = g.up<double>(c->in_a, image, n * 8);
    const uint8_t* dm = mask ? g.up<uint8_t>(c->in_mask, mask, n) : g.out<uint8_t>(c->in_mask, 1);
    if (g.st) return g.st;
    return run_mean(c, di, mask ? dm : nullptr, n, mean);
}

}  // extern "C"
