// multi.cpp -- multi-pair / multi-GPU host layer of libsva.so (include/sva.h,
// "multi-pair batch" and "multi-GPU engine").
//
// Host C++ only.  Pairs are the shard unit: pair j -> device j mod N and
// round-robin over that device's contexts (one HIP stream each), so each
// device keeps its own cost / path volumes and nothing crosses devices until
// the finished u16 disparity maps (and optional f32 sub-pixel maps) are
// gathered to devices[0] -- an RCCL grouped send/recv on a single-process
// communicator (ncclCommInitAll over the engine's devices; librccl is opened
// at sva_multi_create, so libsva.so itself has no RCCL link dependency), or
// peer copies over xGMI (SVA_MULTI_GATHER_PEER).  Every compute step goes
// through the public per-context entry points (sva_disparity_sgm_d,
// sva_fuse_depth_d, and sva_disparity_sgm_conf_d / sva_fuse_depth_conf_d for
// the confidence forms, whose cost planes are gathered like the maps); there
// is no CPU path.  The sva_array_depth* entry points fill one ArrayArgs
// (array_args.h: the arguments and their checks, in one order) and run one
// array_frame(): its jobs are pairs, or -- sva_array_depth_mb -- GROUPS (one
// sva_disparity_sgm_multi_d per reference camera, DESIGN.md §2.2c;
// sva_array_depth_mixed: sva_disparity_sgm_mixed_d, §2.2d), through the same
// plan, slots and gather (run_jobs), depth step and staged download.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "array_args.h"
#include "sva_internal.h"

using namespace sva;

namespace {

// ------------------------------------------------------------ pinned host --
struct PinnedBuf {
    void* ptr = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t n) {
        if (n <= bytes && ptr) return hipSuccess;
        release();
        hipError_t e = hipHostMalloc(&ptr, std::max<size_t>(n, 256), hipHostMallocDefault);
        if (e != hipSuccess) { ptr = nullptr; return e; }
        bytes = std::max<size_t>(n, 256);
        return hipSuccess;
    }
    void release() {
        if (ptr) (void)hipHostFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
};

void copy_plane(uint8_t* dst, const uint8_t* src, int W, int H, size_t pitch) {
    if (pitch == (size_t)W) {
        std::memcpy(dst, src, (size_t)W * H);
        return;
    }
    for (int y = 0; y < H; y++) std::memcpy(dst + (size_t)y * W, src + (size_t)y * pitch, W);
}

// ------------------------------------------------------------------ RCCL --
// The few RCCL entry points the gather uses, resolved from librccl.so.1.
struct Rccl {
    void* lib = nullptr;
    decltype(&ncclCommInitAll) commInitAll = nullptr;
    decltype(&ncclCommDestroy) commDestroy = nullptr;
    decltype(&ncclGroupStart) groupStart = nullptr;
    decltype(&ncclGroupEnd) groupEnd = nullptr;
    decltype(&ncclSend) send = nullptr;
    decltype(&ncclRecv) recv = nullptr;
    decltype(&ncclGetErrorString) errorString = nullptr;

    bool open(std::string& err) {
        const char* names[] = {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"};
        for (const char* n : names)
            if ((lib = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
        if (!lib) {
            err = "cannot load librccl.so.1 (RCCL gather); use SVA_MULTI_GATHER_PEER";
            return false;
        }
#define SVA_SYM(field, name)                                                   \
    field = reinterpret_cast<decltype(field)>(dlsym(lib, name));               \
    if (!field) { err = std::string("librccl lacks ") + name; return false; }
        SVA_SYM(commInitAll, "ncclCommInitAll");
        SVA_SYM(commDestroy, "ncclCommDestroy");
        SVA_SYM(groupStart, "ncclGroupStart");
        SVA_SYM(groupEnd, "ncclGroupEnd");
        SVA_SYM(send, "ncclSend");
        SVA_SYM(recv, "ncclRecv");
        SVA_SYM(errorString, "ncclGetErrorString");
#undef SVA_SYM
        return true;
    }
};

// ---------------------------------------------------------------- engine --
struct Multi {
    std::vector<int> devices;
    int spd = 1;                       // streams (contexts) per device
    int mode = SVA_MULTI_GATHER_RCCL;
    bool gather_all = false;
    std::vector<void*> ctx;            // [d * spd + s]
    std::vector<hipStream_t> copy;     // per device: uploads
    std::vector<hipStream_t> down;     // per device: downloads (device 0 used)
    std::vector<hipEvent_t> gathered;  // per device: last gather done (slot reuse), re-recorded
    bool gathered_valid = false;
    std::vector<std::vector<hipEvent_t>> ev_all;   // per device: per-call events, recycled
    std::vector<size_t> ev_used;
    std::vector<DevBuf> slots;         // per context: local maps of gathered jobs
    std::vector<DevBuf> images;        // per device: uploaded views (sva_array_depth)
    DevBuf maps0, depth0, nvalid0;     // device 0 (sva_array_depth)
    DevBuf conf0, winner0;             // device 0: cost planes, winners (sva_array_depth_conf)
    DevBuf sub0;                       // device 0: f32 sub-pixel maps (sva_array_depth_sub)
    DevBuf cross0;                     // device 0: the checked planes (sva_array_depth_checked)
    DevBuf speckle0;                   // device 0: comp_size planes (sva_array_depth_filtered)
    DevBuf fill0;                      // device 0: n_found planes (sva_array_depth_filled)
    DevBuf wmed0;                      // device 0: the smoothed planes (sva_array_depth_smoothed)
    std::vector<DevBuf> raw, rvalid;   // per device: raw views and the rectified views' valid
                                       // planes, in images' slots (sva_array_depth_rectified)
    PinnedBuf stage_in, stage_out, stage_rect;
    Rccl rccl;
    std::vector<ncclComm_t> comms;
    std::string last_error;

    int nd() const { return (int)devices.size(); }
    Ctx* c(int d, int s) const { return static_cast<Ctx*>(ctx[(size_t)d * spd + s]); }
    hipStream_t st(int d, int s) const { return c(d, s)->stream; }

    int fail(int code, const std::string& m) {
        last_error = m;
        return code;
    }
    int hip_fail(hipError_t e, const char* what) {
        last_error = std::string(what) + ": " + hipGetErrorString(e);
        return (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) ? SVA_ERR_OUT_OF_MEMORY
                                                                          : SVA_ERR_DEVICE;
    }
    int ctx_fail(int code, void* cx, const char* what) {
        last_error = std::string(what) + ": " + sva_last_error(cx);
        return code;
    }
};

#define MHIP(m, expr, what)                                  \
    do {                                                     \
        hipError_t _e = (expr);                              \
        if (_e != hipSuccess) return (m)->hip_fail(_e, what); \
    } while (0)

Multi* as_multi(void* p) { return static_cast<Multi*>(p); }

// A per-call event recorded on device d (recorded events must belong to the
// recording stream's device; any device's stream may wait on them).  Pools are
// reset at the start of each call: a stream wait already enqueued keeps the
// record it captured, so re-recording an event later is safe.
hipError_t ev_on(Multi* m, int d, hipEvent_t* out) {
    hipError_t e = hipSetDevice(m->devices[d]);
    if (e != hipSuccess) return e;
    if (m->ev_used[d] < m->ev_all[d].size()) {
        *out = m->ev_all[d][m->ev_used[d]++];
        return hipSuccess;
    }
    hipEvent_t ev;
    e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) return e;
    m->ev_all[d].push_back(ev);
    m->ev_used[d]++;
    *out = ev;
    return hipSuccess;
}
void ev_reset(Multi* m) { std::fill(m->ev_used.begin(), m->ev_used.end(), 0); }

// `waiter` (on device dw) waits for everything queued so far on `src` (device ds).
int stream_after(Multi* m, int ds, hipStream_t src, hipStream_t waiter) {
    hipEvent_t e;
    MHIP(m, ev_on(m, ds, &e), "event");
    MHIP(m, hipEventRecord(e, src), "event record");
    MHIP(m, hipStreamWaitEvent(waiter, e, 0), "stream wait");
    return SVA_OK;
}

struct Plan {
    std::vector<int32_t> dev, cx, slot;
    std::vector<int> per_ctx;   // jobs per context
};

void make_plan(int nd, int spd, int n, Plan& p) {
    p.dev.resize(n);
    p.cx.resize(n);
    p.slot.resize(n);
    p.per_ctx.assign((size_t)nd * spd, 0);
    for (int j = 0; j < n; j++) {
        p.dev[j] = j % nd;
        p.cx[j] = (j / nd) % spd;
        p.slot[j] = p.per_ctx[(size_t)p.dev[j] * spd + p.cx[j]]++;
    }
}

// Gather job maps living in per-context slots to `dst` on devices[0]:
// dst + j*bytes  <-  slot(j).  `remote[j]` says whether job j needs it.
// All contexts' streams of each device have been joined into st(d, 0).
int gather(Multi* m, const Plan& P, const std::vector<char>& remote,
           const std::vector<const uint8_t*>& src, uint8_t* dst, size_t bytes) {
    const int n = (int)P.dev.size();
    if (m->mode == SVA_MULTI_GATHER_RCCL) {
        ncclResult_t r = m->rccl.groupStart();
        if (r != ncclSuccess) return m->fail(SVA_ERR_DEVICE, m->rccl.errorString(r));
        for (int j = 0; j < n; j++) {
            if (!remote[j]) continue;
            const int d = P.dev[j];
            r = m->rccl.send(src[j], bytes, ncclUint8, 0, m->comms[d], m->st(d, 0));
            if (r == ncclSuccess)
                r = m->rccl.recv(dst + (size_t)j * bytes, bytes, ncclUint8, d, m->comms[0],
                                 m->st(0, 0));
            if (r != ncclSuccess) {
                (void)m->rccl.groupEnd();
                return m->fail(SVA_ERR_DEVICE, std::string("RCCL: ") + m->rccl.errorString(r));
            }
        }
        r = m->rccl.groupEnd();
        if (r != ncclSuccess)
            return m->fail(SVA_ERR_DEVICE, std::string("RCCL: ") + m->rccl.errorString(r));
        return SVA_OK;
    }
    // peer copies, issued on the source device's stream; device 0 joins them
    std::vector<char> used(m->nd(), 0);
    for (int j = 0; j < n; j++) {
        if (!remote[j]) continue;
        const int d = P.dev[j];
        MHIP(m, hipSetDevice(m->devices[d]), "hipSetDevice");
        MHIP(m, hipMemcpyAsync(dst + (size_t)j * bytes, src[j], bytes, hipMemcpyDeviceToDevice,
                               m->st(d, 0)),
             "peer copy");
        used[d] = 1;
    }
    for (int d = 1; d < m->nd(); d++)
        if (used[d]) {
            int s = stream_after(m, d, m->st(d, 0), m->st(0, 0));
            if (s) return s;
        }
    return SVA_OK;
}

// The confidence form of run_pairs: every pair runs
// sva_disparity_sgm_conf_d with this uniqueness, and the planes given here
// (devices[0], [n][H][W] u16, each nullable) are gathered like the maps.  A
// null plane is neither computed into a slot nor shipped.
struct ConfPlanes {
    int uniqueness = 0;
    uint16_t* cost_min = nullptr;
    uint16_t* cost_second = nullptr;
};

// One job's compute call on context cx (its device is current, its waits are
// queued): the map to od, and to os / omin / osec where they are non-null.
using JobCall = std::function<int(int j, void* cx, uint16_t* od, float* os, uint16_t* omin,
                                  uint16_t* osec)>;

// The shared part of sva_batch_sgm_d / sva_array_depth, their confidence forms
// and sva_array_depth_mb: run every job on its context, gather to devices[0].
// A job is whatever `call` computes into one set of [H][W] planes: a pair
// (run_pairs) or a reference camera's whole group (sva_array_depth_mb).
// maps/sub on devices[0] ([n][H][W]); sub may be null, has_sub[j] = job j
// writes one; cp null = no cost planes.
int run_jobs(Multi* m, const Plan& P, const std::vector<std::vector<hipEvent_t>>& wait_for, int W,
             int H, uint16_t* maps, float* sub, const std::vector<char>& has_sub,
             const ConfPlanes* cp, const JobCall& call, const char* what) {
    const int n = (int)P.dev.size();
    const size_t np = (size_t)W * H;
    uint16_t* const cmin = cp ? cp->cost_min : nullptr;
    uint16_t* const csec = cp ? cp->cost_second : nullptr;
    // 0. maps / sub (and the two cost planes) are the caller's buffers on
    // devices[0]: results of the previous call are complete on st(0, 0), and
    // the caller may still be reading them there.  Every stream that writes
    // into them -- device 0's other context streams (local jobs) and, with
    // peer copies, each source device's st(d, 0) -- starts after what is queued
    // on st(0, 0) now.  (The RCCL receives run on st(0, 0) itself.)  The cost
    // planes are written by exactly the streams that write maps (the same
    // job's kernel, the same gather), so these waits order them too.
    {
        hipEvent_t e0;
        MHIP(m, ev_on(m, 0, &e0), "event");
        MHIP(m, hipEventRecord(e0, m->st(0, 0)), "event record");
        for (int s = 1; s < m->spd; s++)
            MHIP(m, hipStreamWaitEvent(m->st(0, s), e0, 0), "stream wait");
        if (m->mode == SVA_MULTI_GATHER_PEER)
            for (int d = 1; d < m->nd(); d++) {
                MHIP(m, hipSetDevice(m->devices[d]), "hipSetDevice");
                MHIP(m, hipStreamWaitEvent(m->st(d, 0), e0, 0), "stream wait");
            }
    }
    // 1. slot workspace per context; a context starts after its device's last gather
    std::vector<char> remote(n, 0);
    for (int j = 0; j < n; j++) remote[j] = P.dev[j] != 0 || m->gather_all;
    // a slot: the map, then the sub-pixel map, cost_min and cost_second where asked for
    // (each plane on a 16-byte boundary, so that an odd W * H keeps the f32 map aligned)
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t off_sub = up16(np * 2), off_min = off_sub + (sub ? up16(np * 4) : 0);
    const size_t off_sec = off_min + (cmin ? up16(np * 2) : 0);
    const size_t per = off_sec + (csec ? up16(np * 2) : 0);
    for (int d = 0; d < m->nd(); d++) {
        MHIP(m, hipSetDevice(m->devices[d]), "hipSetDevice");
        for (int s = 0; s < m->spd; s++) {
            const size_t ci = (size_t)d * m->spd + s;
            if (P.per_ctx[ci] == 0) continue;
            if (d != 0 || m->gather_all) MHIP(m, m->slots[ci].ensure(per * P.per_ctx[ci]), "slots");
            if (m->gathered_valid)
                MHIP(m, hipStreamWaitEvent(m->st(d, s), m->gathered[d], 0), "wait");
        }
    }
    // 2. compute
    std::vector<const uint8_t*> src_map(n, nullptr), src_sub(n, nullptr), src_min(n, nullptr),
        src_sec(n, nullptr);
    for (int j = 0; j < n; j++) {
        const int d = P.dev[j], s = P.cx[j];
        const size_t ci = (size_t)d * m->spd + s;
        uint16_t* od;
        float* os = nullptr;
        uint16_t *omin = nullptr, *osec = nullptr;
        if (remote[j]) {
            uint8_t* base = (uint8_t*)m->slots[ci].ptr + (size_t)P.slot[j] * per;
            od = (uint16_t*)base;
            if (sub) os = (float*)(base + off_sub);
            if (cmin) omin = (uint16_t*)(base + off_min);
            if (csec) osec = (uint16_t*)(base + off_sec);
            src_map[j] = base;
            src_sub[j] = base + off_sub;
            src_min[j] = base + off_min;
            src_sec[j] = base + off_sec;
        } else {
            od = maps + (size_t)j * np;
            if (sub) os = sub + (size_t)j * np;
            if (cmin) omin = cmin + (size_t)j * np;
            if (csec) osec = csec + (size_t)j * np;
        }
        MHIP(m, hipSetDevice(m->devices[d]), "hipSetDevice");
        for (hipEvent_t e : wait_for[j]) MHIP(m, hipStreamWaitEvent(m->st(d, s), e, 0), "wait");
        const int st = call(j, m->ctx[ci], od, os, omin, osec);
        if (st != SVA_OK) return m->ctx_fail(st, m->ctx[ci], what);
    }
    // 3. join each device's streams into its stream 0
    for (int d = 0; d < m->nd(); d++)
        for (int s = 1; s < m->spd; s++) {
            if (P.per_ctx[(size_t)d * m->spd + s] == 0) continue;
            int st = stream_after(m, d, m->st(d, s), m->st(d, 0));
            if (st) return st;
        }
    // 4. gather (maps, then sub-pixel maps, then the cost planes asked for)
    int st = gather(m, P, remote, src_map, (uint8_t*)maps, np * 2);
    if (st) return st;
    if (sub) {
        // only jobs that asked for a sub-pixel map have one (sva.h); the
        // others' planes of `sub` are left untouched, local or remote
        std::vector<char> remote_sub(remote);
        for (int j = 0; j < n; j++) remote_sub[j] = remote[j] && has_sub[j];
        if ((st = gather(m, P, remote_sub, src_sub, (uint8_t*)sub, np * 4))) return st;
    }
    if (cmin && (st = gather(m, P, remote, src_min, (uint8_t*)cmin, np * 2))) return st;
    if (csec && (st = gather(m, P, remote, src_sec, (uint8_t*)csec, np * 2))) return st;
    for (int d = 0; d < m->nd(); d++) {
        MHIP(m, hipSetDevice(m->devices[d]), "hipSetDevice");
        MHIP(m, hipEventRecord(m->gathered[d], m->st(d, 0)), "event record");
    }
    m->gathered_valid = true;
    return SVA_OK;
}

// Pairs as jobs: left/right are per-job device pointers; cp null = the plain
// route (sva_disparity_sgm_d), else sva_disparity_sgm_conf_d.
int run_pairs(Multi* m, const Plan& P, const std::vector<const uint8_t*>& left,
              const std::vector<const uint8_t*>& right, const std::vector<sva_sgm_params>& prm,
              const std::vector<std::vector<hipEvent_t>>& wait_for, int W, int H, size_t pitch,
              uint16_t* maps, float* sub, const ConfPlanes* cp = nullptr) {
    std::vector<char> has_sub(prm.size());
    for (size_t j = 0; j < prm.size(); j++) has_sub[j] = prm[j].subpixel != 0;
    return run_jobs(
        m, P, wait_for, W, H, maps, sub, has_sub, cp,
        [&](int j, void* cx, uint16_t* od, float* os, uint16_t* omin, uint16_t* osec) {
            return cp ? sva_disparity_sgm_conf_d(cx, left[j], right[j], W, H, pitch, &prm[j],
                                                 cp->uniqueness, od, os, omin, osec)
                      : sva_disparity_sgm_d(cx, left[j], right[j], W, H, pitch, &prm[j], od, os);
        },
        "pair");
}

// ------------------------------------------- host batch (sva_batch_sgm) --
// One context's share of sva_batch_sgm: jobs i, i + n, ...; two pipeline
// slots so that upload(j+1) / download(j-1) overlap compute(j).  The lane
// (streams, events, pinned and device staging) lives in the context
// (Ctx::batch_lane) from its first batch to sva_destroy: hipHostMalloc /
// hipFree synchronise the device, so a lane per call cost milliseconds.
struct HostLane {
    Ctx* c = nullptr;
    hipStream_t up = nullptr, dn = nullptr;
    PinnedBuf in[2], out[2];
    DevBuf din[2], dout[2];
    hipEvent_t e_up[2] = {}, e_comp[2] = {}, e_dn[2] = {};
    int job[2] = {-1, -1};
};

int lane_init(HostLane& L) {
    if (hipSetDevice(L.c->device) != hipSuccess) return SVA_ERR_DEVICE;
    if (hipStreamCreateWithFlags(&L.up, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&L.dn, hipStreamNonBlocking) != hipSuccess)
        return SVA_ERR_DEVICE;
    for (int b = 0; b < 2; b++)
        if (hipEventCreateWithFlags(&L.e_up[b], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&L.e_comp[b], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&L.e_dn[b], hipEventDisableTiming) != hipSuccess)
            return SVA_ERR_DEVICE;
    return SVA_OK;
}

void lane_free(HostLane& L) {
    (void)hipSetDevice(L.c->device);
    if (L.up) (void)hipStreamSynchronize(L.up);
    if (L.dn) (void)hipStreamSynchronize(L.dn);
    for (int b = 0; b < 2; b++) {
        L.in[b].release();
        L.out[b].release();
        L.din[b].release();
        L.dout[b].release();
        for (hipEvent_t e : {L.e_up[b], L.e_comp[b], L.e_dn[b]})
            if (e) (void)hipEventDestroy(e);
    }
    if (L.up) (void)hipStreamDestroy(L.up);
    if (L.dn) (void)hipStreamDestroy(L.dn);
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- batch --
int sva_batch_sgm(void** ctxs, int n_ctx, const sva_pair_job* jobs, int n_jobs,
                  const sva_sgm_params* p, int* job_status) {
    if (!ctxs || n_ctx <= 0 || (n_jobs > 0 && !jobs) || n_jobs < 0 || !p)
        return SVA_ERR_INVALID_ARG;
    for (int i = 0; i < n_ctx; i++) {
        if (!ctxs[i]) return SVA_ERR_INVALID_ARG;
        for (int k = 0; k < i; k++)
            if (ctxs[k] == ctxs[i]) return SVA_ERR_INVALID_ARG;   // a context is not re-entrant
    }
    std::vector<int> status(n_jobs, SVA_OK);
    std::vector<std::thread> th;
    for (int i = 0; i < n_ctx; i++) {
        th.emplace_back([&, i]() {
            Ctx* cx = static_cast<Ctx*>(ctxs[i]);
            int s0 = SVA_OK;
            if (!cx->batch_lane) {
                HostLane* nl = new (std::nothrow) HostLane();
                if (!nl) {
                    s0 = SVA_ERR_OUT_OF_MEMORY;
                } else {
                    nl->c = cx;
                    s0 = lane_init(*nl);
                    cx->batch_lane = std::shared_ptr<void>(nl, [](void* q) {
                        HostLane* h = static_cast<HostLane*>(q);
                        lane_free(*h);
                        delete h;
                    });
                    if (s0 != SVA_OK) cx->batch_lane.reset();
                }
            }
            HostLane dummy;
            HostLane& L = cx->batch_lane ? *static_cast<HostLane*>(cx->batch_lane.get()) : dummy;
            L.job[0] = L.job[1] = -1;
            // finish job in slot b: wait for its download, copy out of pinned memory
            auto finish = [&](int b) {
                const int j = L.job[b];
                if (j < 0) return;
                L.job[b] = -1;
                if (hipEventSynchronize(L.e_dn[b]) != hipSuccess) {
                    status[j] = SVA_ERR_DEVICE;
                    return;
                }
                const sva_pair_job& J = jobs[j];
                const size_t np = (size_t)J.width * J.height;
                std::memcpy(J.disp, L.out[b].ptr, np * 2);
                if (J.subpix && p->subpixel)
                    std::memcpy(J.subpix, (uint8_t*)L.out[b].ptr + np * 2, np * 4);
            };
            int q = 0;
            for (int j = i; j < n_jobs; j += n_ctx, q++) {
                if (s0 != SVA_OK) { status[j] = s0; continue; }
                const int b = q & 1;
                finish(b);                                   // job q-2 frees slot b
                const sva_pair_job& J = jobs[j];
                if (!J.left || !J.right || !J.disp || J.width <= 0 || J.height <= 0 ||
                    J.pitch < (size_t)J.width) {
                    status[j] = SVA_ERR_INVALID_ARG;
                    continue;
                }
                const int W = J.width, H = J.height;
                const size_t np = (size_t)W * H;
                const bool want_sub = J.subpix && p->subpixel;
                const size_t out_bytes = np * 2 + (want_sub ? np * 4 : 0);
                if (L.in[b].ensure(np * 2) != hipSuccess ||
                    L.out[b].ensure(out_bytes) != hipSuccess ||
                    L.din[b].ensure(np * 2) != hipSuccess ||
                    L.dout[b].ensure(out_bytes) != hipSuccess) {
                    status[j] = SVA_ERR_OUT_OF_MEMORY;
                    continue;
                }
                uint8_t* pin = (uint8_t*)L.in[b].ptr;
                copy_plane(pin, J.left, W, H, J.pitch);
                copy_plane(pin + np, J.right, W, H, J.pitch);
                uint8_t* d_in = (uint8_t*)L.din[b].ptr;
                uint8_t* d_out = (uint8_t*)L.dout[b].ptr;
                hipError_t e = hipMemcpyAsync(d_in, pin, np * 2, hipMemcpyHostToDevice, L.up);
                if (e == hipSuccess) e = hipEventRecord(L.e_up[b], L.up);
                if (e == hipSuccess) e = hipStreamWaitEvent(L.c->stream, L.e_up[b], 0);
                if (e != hipSuccess) { status[j] = SVA_ERR_DEVICE; continue; }
                const int st = sva_disparity_sgm_d(L.c, d_in, d_in + np, W, H, W, p,
                                                   (uint16_t*)d_out,
                                                   want_sub ? (float*)(d_out + np * 2) : nullptr);
                if (st != SVA_OK) {
                    status[j] = st;
                    (void)hipStreamSynchronize(L.c->stream);
                    continue;
                }
                e = hipEventRecord(L.e_comp[b], L.c->stream);
                if (e == hipSuccess) e = hipStreamWaitEvent(L.dn, L.e_comp[b], 0);
                if (e == hipSuccess)
                    e = hipMemcpyAsync(L.out[b].ptr, d_out, out_bytes, hipMemcpyDeviceToHost, L.dn);
                if (e == hipSuccess) e = hipEventRecord(L.e_dn[b], L.dn);
                if (e != hipSuccess) { status[j] = SVA_ERR_DEVICE; continue; }
                L.job[b] = j;
                // the upload of the next job reuses pinned slot b^1 only after
                // finish(b^1), which waits for that slot's download
            }
            finish(0);
            finish(1);
            // pinned input slots are reused only after their upload completed:
            // e_up precedes e_comp precedes e_dn, which finish() waited on
        });
    }
    for (auto& t : th) t.join();
    int first = SVA_OK;
    for (int j = 0; j < n_jobs; j++) {
        if (job_status) job_status[j] = status[j];
        if (first == SVA_OK && status[j] != SVA_OK) first = status[j];
    }
    return first;
}

// ---------------------------------------------------------------- multi --
int sva_multi_plan(int n_devices, int spd, int n_jobs, int32_t* device_index,
                   int32_t* context_index, int32_t* slot_index) {
    if (n_devices <= 0 || spd <= 0 || n_jobs < 0) return SVA_ERR_INVALID_ARG;
    Plan P;
    make_plan(n_devices, spd, n_jobs, P);
    for (int j = 0; j < n_jobs; j++) {
        if (device_index) device_index[j] = P.dev[j];
        if (context_index) context_index[j] = P.cx[j];
        if (slot_index) slot_index[j] = P.slot[j];
    }
    return SVA_OK;
}

int sva_multi_create(const int* devices, int n_devices, int spd, int flags, void** out) {
    if (!devices || n_devices <= 0 || spd <= 0 || spd > 8 || !out || (flags & ~3))
        return SVA_ERR_INVALID_ARG;
    const int mode = flags & 1;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return SVA_ERR_NO_DEVICE;
    for (int i = 0; i < n_devices; i++) {
        if (devices[i] < 0 || devices[i] >= count) return SVA_ERR_INVALID_ARG;
        for (int k = 0; k < i; k++)
            if (devices[k] == devices[i]) return SVA_ERR_INVALID_ARG;   // one rank per GPU
    }
    Multi* m = new (std::nothrow) Multi();
    if (!m) return SVA_ERR_OUT_OF_MEMORY;
    m->devices.assign(devices, devices + n_devices);
    m->spd = spd;
    m->mode = mode;
    m->gather_all = (flags & SVA_MULTI_GATHER_ALL) != 0;
    m->ctx.assign((size_t)n_devices * spd, nullptr);
    m->slots.resize((size_t)n_devices * spd);
    m->images.resize(n_devices);
    m->raw.resize(n_devices);
    m->rvalid.resize(n_devices);
    m->gathered.assign(n_devices, nullptr);
    m->ev_all.resize(n_devices);
    m->ev_used.assign(n_devices, 0);
    int st = SVA_OK;
    for (int d = 0; d < n_devices && st == SVA_OK; d++) {
        for (int s = 0; s < spd && st == SVA_OK; s++)
            st = sva_create(devices[d], &m->ctx[(size_t)d * spd + s]);
        if (st == SVA_OK && (hipSetDevice(devices[d]) != hipSuccess ||
                             hipEventCreateWithFlags(&m->gathered[d], hipEventDisableTiming) !=
                                 hipSuccess))
            st = SVA_ERR_DEVICE;
    }
    if (st == SVA_OK && mode == SVA_MULTI_GATHER_PEER) {
        for (int d = 1; d < n_devices; d++) {
            int can = 0;
            (void)hipSetDevice(devices[d]);
            if (hipDeviceCanAccessPeer(&can, devices[d], devices[0]) == hipSuccess && can) {
                hipError_t e = hipDeviceEnablePeerAccess(devices[0], 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) st = SVA_ERR_DEVICE;
                (void)hipGetLastError();
            }
        }
    }
    if (st == SVA_OK && mode == SVA_MULTI_GATHER_RCCL) {
        if (!m->rccl.open(m->last_error)) {
            st = SVA_ERR_UNSUPPORTED;
        } else {
            m->comms.assign(n_devices, nullptr);
            ncclResult_t r = m->rccl.commInitAll(m->comms.data(), n_devices, devices);
            if (r != ncclSuccess) st = SVA_ERR_DEVICE;
        }
    }
    if (st != SVA_OK) {
        sva_multi_destroy(m);
        return st;
    }
    *out = m;
    return SVA_OK;
}

int sva_multi_destroy(void* mp) {
    Multi* m = as_multi(mp);
    if (!m) return SVA_ERR_INVALID_ARG;
    for (size_t i = 0; i < m->ctx.size(); i++)
        if (m->ctx[i]) (void)sva_synchronize(m->ctx[i]);
    for (size_t d = 0; d < m->comms.size(); d++)
        if (m->comms[d]) (void)m->rccl.commDestroy(m->comms[d]);
    for (size_t d = 0; d < m->devices.size(); d++) {
        (void)hipSetDevice(m->devices[d]);
        for (int s = 0; s < m->spd; s++) m->slots[d * m->spd + s].release();
        m->images[d].release();
        m->raw[d].release();
        m->rvalid[d].release();
        if (d < m->copy.size() && m->copy[d]) (void)hipStreamDestroy(m->copy[d]);
        if (d < m->down.size() && m->down[d]) (void)hipStreamDestroy(m->down[d]);
    }
    if (!m->devices.empty()) {
        (void)hipSetDevice(m->devices[0]);
        m->maps0.release();
        m->depth0.release();
        m->nvalid0.release();
        m->conf0.release();
        m->winner0.release();
        m->sub0.release();
        m->cross0.release();
        m->speckle0.release();
        m->fill0.release();
        m->wmed0.release();
    }
    m->stage_in.release();
    m->stage_out.release();
    m->stage_rect.release();
    for (size_t d = 0; d < m->devices.size(); d++) {
        (void)hipSetDevice(m->devices[d]);
        if (d < m->ev_all.size())
            for (hipEvent_t e : m->ev_all[d]) (void)hipEventDestroy(e);
        if (d < m->gathered.size() && m->gathered[d]) (void)hipEventDestroy(m->gathered[d]);
    }
    for (void* c : m->ctx)
        if (c) (void)sva_destroy(c);
    if (m->rccl.lib) dlclose(m->rccl.lib);
    delete m;
    return SVA_OK;
}

int sva_multi_synchronize(void* mp) {
    Multi* m = as_multi(mp);
    if (!m) return SVA_ERR_INVALID_ARG;
    for (void* c : m->ctx) {
        const int s = sva_synchronize(c);
        if (s != SVA_OK) return m->ctx_fail(s, c, "synchronize");
    }
    for (size_t d = 0; d < m->copy.size(); d++) {
        MHIP(m, hipSetDevice(m->devices[d]), "hipSetDevice");
        if (m->copy[d]) MHIP(m, hipStreamSynchronize(m->copy[d]), "synchronize");
        if (m->down[d]) MHIP(m, hipStreamSynchronize(m->down[d]), "synchronize");
    }
    return SVA_OK;
}

const char* sva_multi_last_error(void* mp) {
    Multi* m = as_multi(mp);
    return m ? m->last_error.c_str() : "null engine";
}

int sva_multi_context(void* mp, int d, int s, void** out) {
    Multi* m = as_multi(mp);
    if (!m || !out || d < 0 || d >= m->nd() || s < 0 || s >= m->spd) return SVA_ERR_INVALID_ARG;
    *out = m->ctx[(size_t)d * m->spd + s];
    return SVA_OK;
}

}  // extern "C"

namespace {
// sva_batch_sgm_d (cp null) and sva_batch_sgm_conf_d
int batch_sgm_d(void* mp, const sva_pair_d* jobs, int n_jobs, int W, int H, size_t pitch,
                uint16_t* maps, float* sub, const ConfPlanes* cp) {
    Multi* m = as_multi(mp);
    if (!m) return SVA_ERR_INVALID_ARG;
    if (cp && (cp->uniqueness < 0 || cp->uniqueness > 100))
        return m->fail(SVA_ERR_INVALID_ARG, "uniqueness must be 0..100");
    if (n_jobs < 0 || (n_jobs > 0 && (!jobs || !maps)) || W <= 0 || H <= 0 || pitch < (size_t)W)
        return m->fail(SVA_ERR_INVALID_ARG, "bad batch arguments");
    if (n_jobs == 0) return SVA_OK;
    bool any_sub = false;
    for (int j = 0; j < n_jobs; j++) {
        if (!jobs[j].left || !jobs[j].right || check_params(jobs[j].params))
            return m->fail(SVA_ERR_INVALID_ARG, "bad pair " + std::to_string(j));
        any_sub |= jobs[j].params.subpixel != 0;
    }
    ev_reset(m);
    Plan P;
    make_plan(m->nd(), m->spd, n_jobs, P);
    std::vector<const uint8_t*> l(n_jobs), r(n_jobs);
    std::vector<sva_sgm_params> prm(n_jobs);
    std::vector<std::vector<hipEvent_t>> none(n_jobs);
    for (int j = 0; j < n_jobs; j++) {
        l[j] = jobs[j].left;
        r[j] = jobs[j].right;
        prm[j] = jobs[j].params;
    }
    return run_pairs(m, P, l, r, prm, none, W, H, pitch, maps, any_sub ? sub : nullptr, cp);
}

// The host views of an array frame onto the devices that need them
// (sva_array_depth*): pair j runs on device dev_of[j].  Out: slot_of[d][v], the
// slot of view v in m->images[d] (-1: not needed there), and up_ev[d][v], the
// event of its upload on the device's copy stream.  plan_views (array_args.h)
// decides who needs what; refs_on_0: every reference view on device 0 too.
// rect (sva_array_depth_rectified; null for every other entry): the host views
// are RAW.  They land in m->raw[d], one sva_rectify_d launch per device on its
// copy stream writes the slots of m->images[d] -- and, where a mask or valid_out
// needs them, of m->rvalid[d] -- and up_ev[d][v] is recorded after that launch.
// views_out / valid_out are copied out here, from the first device that has the
// view, before this returns.
int upload_views(Multi* m, const uint8_t* const* images, int n_images, int W, int H, size_t pitch,
                 const sva_array_pair* pairs, int n_pairs, const std::vector<int32_t>& dev_of,
                 bool refs_on_0, const ArrayArgs* rect, std::vector<std::vector<int>>& slot_of,
                 std::vector<std::vector<hipEvent_t>>& up_ev) {
    const size_t np = (size_t)W * H;
    if (m->copy.empty()) {
        m->copy.assign(m->nd(), nullptr);
        m->down.assign(m->nd(), nullptr);
        for (int d = 0; d < m->nd(); d++) {
            MHIP(m, hipSetDevice(m->devices[d]), "hipSetDevice");
            MHIP(m, hipStreamCreateWithFlags(&m->copy[d], hipStreamNonBlocking), "stream");
            MHIP(m, hipStreamCreateWithFlags(&m->down[d], hipStreamNonBlocking), "stream");
        }
    }
    // 1. which views each device needs, staged once into pinned memory
    std::vector<int> n_need;
    std::vector<char> used;
    plan_views(m->nd(), n_images, pairs, n_pairs, dev_of.data(), refs_on_0, slot_of, n_need, used);
    std::vector<int> pin_slot(n_images, -1);
    int n_pin = 0;
    for (int v = 0; v < n_images; v++)
        if (used[v]) pin_slot[v] = n_pin++;
    // the previous call's uploads must be done before the pinned staging is rewritten
    for (int d = 0; d < m->nd(); d++) {
        MHIP(m, hipSetDevice(m->devices[d]), "hipSetDevice");
        MHIP(m, hipStreamSynchronize(m->copy[d]), "synchronize");
    }
    MHIP(m, m->stage_in.ensure((size_t)n_pin * np), "pinned staging");
    // 2. uploads on each device's copy stream, one event per (device, view);
    // the images buffer is reused only after the previous call's pairs ran
    up_ev.assign(m->nd(), std::vector<hipEvent_t>(n_images));
    for (int v = 0; v < n_images; v++)
        if (used[v])
            copy_plane((uint8_t*)m->stage_in.ptr + (size_t)pin_slot[v] * np, images[v], W, H, pitch);
    for (int d = 0; d < m->nd(); d++) {
        if (!n_need[d]) continue;
        MHIP(m, hipSetDevice(m->devices[d]), "hipSetDevice");
        for (int s = 0; s < m->spd; s++) {
            int st = stream_after(m, d, m->st(d, s), m->copy[d]);
            if (st) return st;
        }
        MHIP(m, m->images[d].ensure((size_t)n_need[d] * np), "view workspace");
        if (rect) MHIP(m, m->raw[d].ensure((size_t)n_need[d] * np), "raw view workspace");
        uint8_t* land = (uint8_t*)(rect ? m->raw[d].ptr : m->images[d].ptr);
        for (int v = 0; v < n_images; v++) {
            if (slot_of[d][v] < 0) continue;
            MHIP(m, hipMemcpyAsync(land + (size_t)slot_of[d][v] * np,
                                   (uint8_t*)m->stage_in.ptr + (size_t)pin_slot[v] * np, np,
                                   hipMemcpyHostToDevice, m->copy[d]),
                 "upload");
            if (rect) continue;
            MHIP(m, ev_on(m, d, &up_ev[d][v]), "event");
            MHIP(m, hipEventRecord(up_ev[d][v], m->copy[d]), "event record");
        }
    }
    if (!rect) return SVA_OK;
    // 3. one rectify launch per device behind its uploads, through the device's
    // first context with the copy stream as its stream; one event for all its views
    std::vector<int> home(n_images, -1);   // the first device that has the view
    const bool want_out = rect->views_out || rect->valid_out;
    if (want_out) MHIP(m, m->stage_rect.ensure((size_t)n_pin * np * 2), "pinned staging");
    for (int d = 0; d < m->nd(); d++) {
        if (!n_need[d]) continue;
        MHIP(m, hipSetDevice(m->devices[d]), "hipSetDevice");
        const bool want_valid = (d == 0 && rect->rect_mask) || rect->valid_out;
        if (want_valid) MHIP(m, m->rvalid[d].ensure((size_t)n_need[d] * np), "valid workspace");
        std::vector<sva_rectify_view> table(n_need[d]);
        for (int v = 0; v < n_images; v++)
            if (slot_of[d][v] >= 0) table[slot_of[d][v]] = rect->rect_views[v];
        Ctx* c = m->c(d, 0);
        const hipStream_t own = c->stream;
        c->stream = m->copy[d];
        const int st = sva_rectify_d(c, (const uint8_t*)m->raw[d].ptr, n_need[d], W, H, (size_t)W,
                                     table.data(), W, H, (size_t)W, rect->rect_border,
                                     (uint8_t*)m->images[d].ptr,
                                     want_valid ? (uint8_t*)m->rvalid[d].ptr : nullptr, nullptr);
        c->stream = own;
        if (st) return m->ctx_fail(st, c, "rectify");
        hipEvent_t done;
        MHIP(m, ev_on(m, d, &done), "event");
        MHIP(m, hipEventRecord(done, m->copy[d]), "event record");
        for (int v = 0; v < n_images; v++) {
            if (slot_of[d][v] < 0) continue;
            up_ev[d][v] = done;
            if (!want_out || home[v] >= 0) continue;
            home[v] = d;
            uint8_t* pin = (uint8_t*)m->stage_rect.ptr + (size_t)pin_slot[v] * np * 2;
            const size_t at = (size_t)slot_of[d][v] * np;
            if (rect->views_out)
                MHIP(m, hipMemcpyAsync(pin, (uint8_t*)m->images[d].ptr + at, np,
                                       hipMemcpyDeviceToHost, m->copy[d]), "download");
            if (rect->valid_out)
                MHIP(m, hipMemcpyAsync(pin + np, (uint8_t*)m->rvalid[d].ptr + at, np,
                                       hipMemcpyDeviceToHost, m->copy[d]), "download");
        }
    }
    for (int d = 0; want_out && d < m->nd(); d++) {
        if (!n_need[d]) continue;
        MHIP(m, hipSetDevice(m->devices[d]), "hipSetDevice");
        MHIP(m, hipStreamSynchronize(m->copy[d]), "synchronize");
    }
    for (int v = 0; want_out && v < n_images; v++) {
        if (home[v] < 0) continue;
        const uint8_t* pin = (const uint8_t*)m->stage_rect.ptr + (size_t)pin_slot[v] * np * 2;
        if (rect->views_out) std::memcpy(rect->views_out + (size_t)v * np, pin, np);
        if (rect->valid_out) std::memcpy(rect->valid_out + (size_t)v * np, pin + np, np);
    }
    return SVA_OK;
}

// The staged download of a frame's outputs.  Each plane asked for (dst
// non-null) is registered as (device source, host destination, bytes) with the
// step it follows and gets the next place in stage_out; queue() copies a
// step's planes there on down[0], finish() synchronises and copies them out.
struct Download {
    struct Plane { const void* src; void* dst; size_t bytes, off; int step; };
    std::vector<Plane> planes;
    size_t total = 0;

    void add(int step, const void* src, void* dst, size_t bytes) {
        if (!dst) return;
        planes.push_back({src, dst, bytes, total, step});
        total += bytes;
    }
    int queue(Multi* m, int step) const {
        for (const Plane& p : planes)
            if (p.step == step)
                MHIP(m, hipMemcpyAsync((uint8_t*)m->stage_out.ptr + p.off, p.src, p.bytes,
                                       hipMemcpyDeviceToHost, m->down[0]),
                     "download");
        return SVA_OK;
    }
    int finish(Multi* m) const {
        MHIP(m, hipStreamSynchronize(m->down[0]), "synchronize");
        for (const Plane& p : planes)
            std::memcpy(p.dst, (const uint8_t*)m->stage_out.ptr + p.off, p.bytes);
        return SVA_OK;
    }
};

// One camera-array frame, behind every sva_array_depth* entry (array_args.h has
// their arguments and checks).  A job is a pair (ArrayRoute::Pairs: every
// pair through sva_disparity_sgm_d or, with conf, sva_disparity_sgm_conf_d; a
// group's maps are fused by `mode`) or a GROUP (group g's
// pairs go through one sva_disparity_sgm_multi_d on device g mod n_devices,
// and its one map becomes depth at the group's baseline; GroupsMixed, §2.2d:
// sva_disparity_sgm_mixed_d, and the depth scale is the unit baseline).  With
// a.sub (sva_array_depth_sub, §2.6c) every job also writes its f32 sub-pixel
// map, gathered into sub0 like the u16 one, and depth is fused from those.
// With a.cross (sva_array_depth_checked, §2.5b) the groups' maps pass through
// sva_cross_check_d on device 0 before step 4, which then reads the checked
// planes.  With a.speckle (sva_array_depth_filtered, §2.5c) every job's map --
// checked or not -- then passes through sva_filter_speckles_d in place, and
// with a.fill (sva_array_depth_filled, §2.5d) through sva_fill_holes_d after it,
// and with a.wmed (sva_array_depth_smoothed, §2.5e) through sva_weighted_median_d.
// With a.rect (sva_array_depth_rectified, §2.5f) the views are raw: upload_views
// rectifies them, and with a.rect_mask step 3a masks the gathered maps.
int array_frame(void* mp, const ArrayArgs& a) {
    Multi* m = as_multi(mp);
    if (!m) return SVA_ERR_INVALID_ARG;
    std::string msg;
    std::vector<int32_t> ratio;   // GroupsMixed: every pair's (num, den)
    if (int st = check_array_args(a, msg, ratio)) return m->fail(st, msg);
    const bool group = a.route != ArrayRoute::Pairs;
    const int W = a.W, H = a.H, n_pairs = a.n_pairs, n_groups = a.n_groups;
    const int n_jobs = group ? n_groups : n_pairs;
    const sva_array_pair* pairs = a.pairs;
    const int32_t* gs = a.group_start;
    ev_reset(m);
    const size_t np = (size_t)W * H;
    Plan P;
    make_plan(m->nd(), m->spd, n_jobs, P);
    // job k is pairs[first[k] .. first[k + 1])
    std::vector<int32_t> first(n_jobs + 1), dev_of(n_pairs);
    for (int k = 0; k <= n_jobs; k++) first[k] = group ? gs[k] : k;
    for (int k = 0; k < n_jobs; k++)
        for (int j = first[k]; j < first[k + 1]; j++) dev_of[j] = P.dev[k];
    // 1-2. the views each device needs, uploaded on its copy stream
    std::vector<std::vector<int>> slot_of;
    std::vector<std::vector<hipEvent_t>> up_ev;
    if (int st = upload_views(m, a.images, a.n_images, W, H, a.pitch, pairs, n_pairs, dev_of,
                              a.wmed || (a.rect && a.rect_mask), a.rect ? &a : nullptr, slot_of,
                              up_ev))
        return st;
    // 3. jobs + gather into maps0 on device 0
    MHIP(m, hipSetDevice(m->devices[0]), "hipSetDevice");
    MHIP(m, hipStreamSynchronize(m->st(0, 0)), "synchronize");   // maps0/depth0 reuse
    const size_t plane = np * 2 * n_jobs;
    MHIP(m, m->maps0.ensure(plane), "map workspace");
    MHIP(m, m->depth0.ensure(np * 8 * n_groups), "depth workspace");
    if (!group) MHIP(m, m->nvalid0.ensure(np * n_groups), "depth workspace");
    // the cost planes the fusion mode reads, and those the caller asked for
    const bool want_min = a.conf && (a.mode != SVA_FUSE_MEDIAN || a.cost_min);
    const bool want_sec = a.conf && (a.mode == SVA_FUSE_MAX_MARGIN || a.cost_second);
    if (want_min || want_sec)
        MHIP(m, m->conf0.ensure(plane * ((want_min ? 1 : 0) + (want_sec ? 1 : 0))), "cost planes");
    if (a.winner) MHIP(m, m->winner0.ensure(np * n_groups), "winner workspace");
    if (a.sub) MHIP(m, m->sub0.ensure(plane * 2), "sub-pixel workspace");
    uint16_t* maps0 = (uint16_t*)m->maps0.ptr;
    float* sub0 = a.sub ? (float*)m->sub0.ptr : nullptr;
    ConfPlanes cp;
    cp.uniqueness = a.uniqueness;
    cp.cost_min = want_min ? (uint16_t*)m->conf0.ptr : nullptr;
    cp.cost_second = want_sec ? (uint16_t*)m->conf0.ptr + (want_min ? np * n_jobs : 0) : nullptr;
    // per job: its reference view, its matched views and steps, its uploads
    std::vector<const uint8_t*> ref(n_jobs);
    std::vector<std::vector<const uint8_t*>> others(n_jobs);
    std::vector<std::vector<int32_t>> steps(n_jobs);
    std::vector<sva_sgm_params> prm(n_jobs);
    std::vector<std::vector<hipEvent_t>> waits(n_jobs);
    for (int k = 0; k < n_jobs; k++) {
        const int d = P.dev[k], j0 = first[k];
        const uint8_t* base = (const uint8_t*)m->images[d].ptr;
        ref[k] = base + (size_t)slot_of[d][pairs[j0].ref] * np;
        waits[k].push_back(up_ev[d][pairs[j0].ref]);
        for (int j = j0; j < first[k + 1]; j++) {
            others[k].push_back(base + (size_t)slot_of[d][pairs[j].other] * np);
            steps[k].push_back(pairs[j].params.dir);
            steps[k].push_back(pairs[j].params.dir_y);
            waits[k].push_back(up_ev[d][pairs[j].other]);
        }
        prm[k] = pairs[j0].params;
        prm[k].subpixel = a.sub ? 1 : 0;
    }
    // os: the job's plane of sub0, null for every entry but sva_array_depth_sub
    int st = run_jobs(
        m, P, waits, W, H, maps0, sub0, std::vector<char>(n_jobs, a.sub ? 1 : 0),
        a.conf ? &cp : nullptr,
        [&](int k, void* cx, uint16_t* od, float* os, uint16_t* omin, uint16_t* osec) {
            const int n = (int)others[k].size();
            switch (a.route) {
                case ArrayRoute::GroupsMixed:
                    return sva_disparity_sgm_mixed_d(cx, ref[k], others[k].data(), steps[k].data(),
                                                     &ratio[2 * (size_t)first[k]], n, W, H, W,
                                                     &prm[k], a.uniqueness, od, os, omin, osec);
                case ArrayRoute::Groups:
                    return sva_disparity_sgm_multi_d(cx, ref[k], others[k].data(), steps[k].data(),
                                                     n, W, H, W, &prm[k], a.uniqueness, od, os,
                                                     omin, osec);
                default:
                    return a.conf ? sva_disparity_sgm_conf_d(cx, ref[k], others[k][0], W, H, W,
                                                             &prm[k], a.uniqueness, od, os, omin,
                                                             osec)
                                  : sva_disparity_sgm_d(cx, ref[k], others[k][0], W, H, W, &prm[k],
                                                        od, os);
            }
        },
        group ? "group" : "pair");
    if (st) return st;
    // 3a. the mask of a frame from raw views: every job's map (and f32 map), in
    // place, by the valid plane of its reference view on device 0
    if (a.rect && a.rect_mask) {
        MHIP(m, hipSetDevice(m->devices[0]), "hipSetDevice");
        for (int k = 0; k < n_jobs; k++) {
            const int v = pairs[first[k]].ref;
            const size_t o = (size_t)k * np;
            MHIP(m, hipStreamWaitEvent(m->st(0, 0), up_ev[0][v], 0), "wait");
            st = sva_mask_maps_d(m->ctx[0], maps0 + o, sub0 ? sub0 + o : nullptr, 1, W, H,
                                 (const uint8_t*)m->rvalid[0].ptr + (size_t)slot_of[0][v] * np,
                                 pairs[first[k]].params.invalid, maps0 + o,
                                 sub0 ? sub0 + o : nullptr);
            if (st) return m->ctx_fail(st, m->ctx[0], "mask");
        }
    }
    // 3b. the cross-view check: one pass on device 0 over the gathered maps into
    // planes of cross0 -- u16 maps, f32 maps (sub), agree, conflict -- which take
    // the place of maps0 / sub0 from here on
    uint8_t *agree0 = nullptr, *conflict0 = nullptr;
    if (a.cross) {
        MHIP(m, hipSetDevice(m->devices[0]), "hipSetDevice");
        MHIP(m, m->cross0.ensure(plane * (a.sub ? 3 : 1) + 2 * np * n_groups), "check workspace");
        uint8_t* w = (uint8_t*)m->cross0.ptr;
        float* csub = a.sub ? (float*)w : nullptr;             // the f32 planes first: aligned
        uint16_t* cmaps = (uint16_t*)(w + (a.sub ? plane * 2 : 0));
        agree0 = w + plane * (a.sub ? 3 : 1);
        conflict0 = agree0 + np * n_groups;
        std::vector<int32_t> vs(2 * (size_t)n_groups);
        for (int g = 0; g < n_groups; g++) {
            vs[2 * (size_t)g] = a.view_step[2 * pairs[gs[g]].ref];
            vs[2 * (size_t)g + 1] = a.view_step[2 * pairs[gs[g]].ref + 1];
        }
        st = sva_cross_check_d(m->ctx[0], maps0, sub0, n_groups, W, H, vs.data(),
                               pairs[0].params.invalid, a.max_diff, a.min_agree, a.max_conflict,
                               cmaps, csub, agree0, conflict0);
        if (st) return m->ctx_fail(st, m->ctx[0], "cross-view check");
        maps0 = cmaps;
        sub0 = csub;
    }
    // 3c. the speckle filter, in place on the maps step 4 reads: one call per run
    // of jobs that share `invalid` (a pair route's groups may differ in it)
    uint32_t* size0 = nullptr;
    if (a.speckle) {
        MHIP(m, hipSetDevice(m->devices[0]), "hipSetDevice");
        if (a.comp_size) {
            MHIP(m, m->speckle0.ensure(plane * 2), "speckle workspace");
            size0 = (uint32_t*)m->speckle0.ptr;
        }
        for (int k = 0, k1; k < n_jobs; k = k1) {
            const uint16_t inv = pairs[first[k]].params.invalid;
            for (k1 = k + 1; k1 < n_jobs && pairs[first[k1]].params.invalid == inv;) k1++;
            const size_t o = (size_t)k * np;
            float* sk = sub0 ? sub0 + o : nullptr;
            st = sva_filter_speckles_d(m->ctx[0], maps0 + o, sk, k1 - k, W, H, inv,
                                       a.speckle_max_size, a.speckle_max_diff, maps0 + o, sk,
                                       size0 ? size0 + o : nullptr);
            if (st) return m->ctx_fail(st, m->ctx[0], "speckle filter");
        }
    }
    // 3d. hole filling, in place on the same maps (and f32 maps): one call per
    // run of at most kFillFrameMaps jobs that share `invalid`, which bounds the
    // context's key planes
    uint8_t* found0 = nullptr;
    if (a.fill) {
        MHIP(m, hipSetDevice(m->devices[0]), "hipSetDevice");
        // the plane is kept for step 3e's select even if the caller did not ask for it
        if (a.n_found || (a.wmed && a.wmed_select == 1)) {
            MHIP(m, m->fill0.ensure(np * n_jobs), "fill workspace");
            found0 = (uint8_t*)m->fill0.ptr;
        }
        for (int k = 0, k1; k < n_jobs; k = k1) {
            const uint16_t inv = pairs[first[k]].params.invalid;
            for (k1 = k + 1; k1 < n_jobs && k1 - k < tune::kFillFrameMaps &&
                             pairs[first[k1]].params.invalid == inv;)
                k1++;
            const size_t o = (size_t)k * np;
            float* sk = sub0 ? sub0 + o : nullptr;
            st = sva_fill_holes_d(m->ctx[0], maps0 + o, sk, k1 - k, W, H, inv, a.fill_max_dist,
                                  a.fill_min_found, a.fill_mode, maps0 + o, sk,
                                  found0 ? found0 + o : nullptr);
            if (st) return m->ctx_fail(st, m->ctx[0], "hole filling");
        }
    }
    // 3e. the weighted median filter, guided by each job's reference view on
    // device 0, into planes of wmed0 -- f32 maps (sub), u16 maps, support -- which
    // take the place of maps0 / sub0 from here on: one call per run of jobs that
    // share `invalid`
    uint16_t* support0 = nullptr;
    if (a.wmed) {
        MHIP(m, hipSetDevice(m->devices[0]), "hipSetDevice");
        MHIP(m, m->wmed0.ensure(plane * (a.sub ? 3 : 1) + (a.support ? plane : 0)), "wmed workspace");
        uint8_t* w = (uint8_t*)m->wmed0.ptr;
        float* wsub = a.sub ? (float*)w : nullptr;             // the f32 planes first: aligned
        uint16_t* wmaps = (uint16_t*)(w + (a.sub ? plane * 2 : 0));
        if (a.support) support0 = wmaps + np * n_jobs;
        std::vector<const uint8_t*> guides(n_jobs);
        for (int k = 0; k < n_jobs; k++) {
            const int v = pairs[first[k]].ref;
            guides[k] = (const uint8_t*)m->images[0].ptr + (size_t)slot_of[0][v] * np;
            if (a.wmed_weights)
                MHIP(m, hipStreamWaitEvent(m->st(0, 0), up_ev[0][v], 0), "wait");
        }
        const uint8_t* sel0 = a.wmed_select == 1 ? found0 : nullptr;
        for (int k = 0, k1; k < n_jobs; k = k1) {
            const uint16_t inv = pairs[first[k]].params.invalid;
            for (k1 = k + 1; k1 < n_jobs && pairs[first[k1]].params.invalid == inv;) k1++;
            const size_t o = (size_t)k * np;
            st = sva_weighted_median_d(m->ctx[0], maps0 + o, sub0 ? sub0 + o : nullptr,
                                       a.wmed_weights ? guides.data() + k : nullptr, (size_t)W,
                                       a.wmed_weights, sel0 ? sel0 + o : nullptr, k1 - k, W, H, inv,
                                       a.wmed_radius, a.wmed_min_support, 1, wmaps + o,
                                       wsub ? wsub + o : nullptr, support0 ? support0 + o : nullptr);
            if (st) return m->ctx_fail(st, m->ctx[0], "weighted median");
        }
        maps0 = wmaps;
        sub0 = wsub;
    }
    // 4. depth per group on device 0 -- the fusion of its pairs' maps, or the
    // depth of its one map (the median of one is the map's own depth) -- each
    // group's download as soon as it is done, the per-job planes at the end
    MHIP(m, hipSetDevice(m->devices[0]), "hipSetDevice");
    double* depth0 = (double*)m->depth0.ptr;
    uint8_t* nv0 = group ? nullptr : (uint8_t*)m->nvalid0.ptr;
    uint8_t* win0 = a.winner ? (uint8_t*)m->winner0.ptr : nullptr;
    Download dl;
    for (int g = 0; g < n_groups; g++) {
        const size_t o = (size_t)g * np;
        dl.add(g, depth0 + o, a.depth + o, np * 8);
        if (nv0 && a.n_valid) dl.add(g, nv0 + o, a.n_valid + o, np);
        if (win0) dl.add(g, win0 + o, a.winner + o, np);
    }
    dl.add(n_groups, maps0, a.maps, plane);
    dl.add(n_groups, sub0, a.subpix, plane * 2);
    dl.add(n_groups, cp.cost_min, a.cost_min, plane);
    dl.add(n_groups, cp.cost_second, a.cost_second, plane);
    dl.add(n_groups, agree0, a.agree, np * n_groups);
    dl.add(n_groups, conflict0, a.conflict, np * n_groups);
    dl.add(n_groups, size0, a.comp_size, plane * 2);
    dl.add(n_groups, found0, a.n_found, np * n_jobs);
    dl.add(n_groups, support0, a.support, plane);
    MHIP(m, m->stage_out.ensure(dl.total), "pinned staging");
    std::vector<double> bases(n_pairs);
    for (int j = 0; j < n_pairs; j++) bases[j] = pairs[j].baseline;
    for (int g = 0; g < n_groups; g++) {
        const int j0 = gs[g];
        const size_t o = (size_t)g * np, o_maps = (size_t)(group ? g : j0) * np;
        const int n_maps = group ? 1 : gs[g + 1] - j0;
        const double* base =
            a.route == ArrayRoute::GroupsMixed ? &a.unit_baseline[g] : &bases[j0];
        const bool by_cost = a.conf && a.mode != SVA_FUSE_MEDIAN;
        if (a.sub && by_cost)
            st = sva_fuse_depth_conf_sub_d(m->ctx[0], maps0 + o_maps, sub0 + o_maps,
                                           cp.cost_min + o_maps,
                                           cp.cost_second ? cp.cost_second + o_maps : nullptr,
                                           n_maps, W, H, base, a.f, a.pixel_size,
                                           pairs[j0].params.invalid, a.mode, depth0 + o,
                                           nv0 ? nv0 + o : nullptr, win0 ? win0 + o : nullptr);
        else if (a.sub)
            st = sva_fuse_depth_sub_d(m->ctx[0], maps0 + o_maps, sub0 + o_maps, n_maps, W, H, base,
                                      a.f, a.pixel_size, pairs[j0].params.invalid, depth0 + o,
                                      nv0 ? nv0 + o : nullptr);
        else if (by_cost)
            st = sva_fuse_depth_conf_d(m->ctx[0], maps0 + o_maps, cp.cost_min + o_maps,
                                       cp.cost_second ? cp.cost_second + o_maps : nullptr, n_maps,
                                       W, H, base, a.f, a.pixel_size, pairs[j0].params.invalid,
                                       a.mode, depth0 + o, nv0 ? nv0 + o : nullptr,
                                       win0 ? win0 + o : nullptr);
        else
            st = sva_fuse_depth_d(m->ctx[0], maps0 + o_maps, n_maps, W, H, base, a.f, a.pixel_size,
                                  pairs[j0].params.invalid, depth0 + o, nv0 ? nv0 + o : nullptr);
        if (st) return m->ctx_fail(st, m->ctx[0], group ? "depth" : "fuse");
        if ((st = stream_after(m, 0, m->st(0, 0), m->down[0]))) return st;
        if ((st = dl.queue(m, g))) return st;
    }
    if ((st = dl.queue(m, n_groups))) return st;
    return dl.finish(m);
}

// What every entry point shares; as it stands, sva_array_depth's: the pair
// route, plain matching, median fusion.
ArrayArgs frame_args(const uint8_t* const* images, int n_images, int W, int H, size_t pitch,
                     const sva_array_pair* pairs, int n_pairs, const int32_t* group_start,
                     int n_groups, double f, double pixel_size, int uniqueness, double* depth,
                     uint16_t* maps, uint16_t* cost_min, uint16_t* cost_second) {
    ArrayArgs a;
    a.images = images;
    a.n_images = n_images;
    a.W = W;
    a.H = H;
    a.pitch = pitch;
    a.pairs = pairs;
    a.n_pairs = n_pairs;
    a.group_start = group_start;
    a.n_groups = n_groups;
    a.f = f;
    a.pixel_size = pixel_size;
    a.uniqueness = uniqueness;
    a.depth = depth;
    a.maps = maps;
    a.cost_min = cost_min;
    a.cost_second = cost_second;
    return a;
}

// frame_args and the arguments of the entries that take a route
// (sva_array_depth_sub and the four after it): the confidence instance, `mode`
// as given.  Then one setter per argument group of the post-filter chain.
ArrayArgs routed_args(const uint8_t* const* images, int n_images, int W, int H, size_t pitch,
                      const sva_array_pair* pairs, int n_pairs, const int32_t* group_start,
                      int n_groups, int route, const double* unit_baseline, double f,
                      double pixel_size, int uniqueness, int mode, double* depth, uint8_t* n_valid,
                      uint8_t* winner, float* subpix, uint16_t* maps, uint16_t* cost_min,
                      uint16_t* cost_second) {
    ArrayArgs a = frame_args(images, n_images, W, H, pitch, pairs, n_pairs, group_start, n_groups,
                             f, pixel_size, uniqueness, depth, maps, cost_min, cost_second);
    a.route = array_route_of(route);
    a.conf = true;
    a.mode = mode;
    a.unit_baseline = unit_baseline;
    a.n_valid = n_valid;
    a.winner = winner;
    a.subpix = subpix;
    return a;
}

// on = false (check = 0) ignores the check's arguments; the planes stay, for
// check_array_args to refuse.
void set_cross(ArrayArgs& a, bool on, const int32_t* view_step, int max_diff, int min_agree,
               int max_conflict, uint8_t* agree, uint8_t* conflict) {
    a.cross = on;
    if (on) {
        a.view_step = view_step;
        a.max_diff = max_diff;
        a.min_agree = min_agree;
        a.max_conflict = max_conflict;
    }
    a.agree = agree;
    a.conflict = conflict;
}

void set_speckle(ArrayArgs& a, int check, int max_size, int max_diff, uint32_t* comp_size) {
    a.speckle = true;
    a.check = check;
    a.speckle_max_size = max_size;
    a.speckle_max_diff = max_diff;
    a.comp_size = comp_size;
}

// (an entry without the fill does not call this: its arguments keep their defaults)
void set_fill(ArrayArgs& a, int max_dist, int min_found, int mode, uint8_t* n_found) {
    a.fill = true;
    a.fill_max_dist = max_dist;
    a.fill_min_found = min_found;
    a.fill_mode = mode;
    a.n_found = n_found;
}

void set_wmed(ArrayArgs& a, int radius, const uint16_t* weights, int min_support, int select,
              uint16_t* support) {
    a.wmed = true;
    a.wmed_radius = radius;
    a.wmed_weights = weights;
    a.wmed_min_support = min_support;
    a.wmed_select = select;
    a.support = support;
}

// The frame of an entry that takes `sub` as a number: one outside 0 / 1 is
// refused here, before it becomes ArrayArgs::sub, whatever else is wrong.
int sub_frame(void* mp, ArrayArgs& a, int sub) {
    if (sub != 0 && sub != 1) {
        Multi* m = as_multi(mp);
        return m ? m->fail(SVA_ERR_INVALID_ARG, "sub must be 0 or 1") : SVA_ERR_INVALID_ARG;
    }
    a.sub = sub != 0;
    return array_frame(mp, a);
}
}  // namespace

extern "C" {

int sva_batch_sgm_d(void* mp, const sva_pair_d* jobs, int n_jobs, int W, int H, size_t pitch,
                    uint16_t* maps, float* sub) {
    return batch_sgm_d(mp, jobs, n_jobs, W, H, pitch, maps, sub, nullptr);
}

int sva_batch_sgm_conf_d(void* mp, const sva_pair_d* jobs, int n_jobs, int W, int H, size_t pitch,
                         int uniqueness, uint16_t* maps, float* sub, uint16_t* cost_min,
                         uint16_t* cost_second) {
    ConfPlanes cp;
    cp.uniqueness = uniqueness;
    cp.cost_min = cost_min;
    cp.cost_second = cost_second;
    return batch_sgm_d(mp, jobs, n_jobs, W, H, pitch, maps, sub, &cp);
}

int sva_array_depth(void* mp, const uint8_t* const* images, int n_images, int W, int H,
                    size_t pitch, const sva_array_pair* pairs, int n_pairs,
                    const int32_t* group_start, int n_groups, double f, double pixel_size,
                    double* depth, uint8_t* n_valid, uint16_t* maps) {
    ArrayArgs a = frame_args(images, n_images, W, H, pitch, pairs, n_pairs, group_start, n_groups,
                             f, pixel_size, 0, depth, maps, nullptr, nullptr);
    a.n_valid = n_valid;
    return array_frame(mp, a);
}

int sva_array_depth_conf(void* mp, const uint8_t* const* images, int n_images, int W, int H,
                         size_t pitch, const sva_array_pair* pairs, int n_pairs,
                         const int32_t* group_start, int n_groups, double f, double pixel_size,
                         int uniqueness, int mode, double* depth, uint8_t* n_valid,
                         uint8_t* winner, uint16_t* maps, uint16_t* cost_min,
                         uint16_t* cost_second) {
    ArrayArgs a = frame_args(images, n_images, W, H, pitch, pairs, n_pairs, group_start, n_groups,
                             f, pixel_size, uniqueness, depth, maps, cost_min, cost_second);
    a.conf = true;
    a.mode = mode;
    a.n_valid = n_valid;
    a.winner = winner;
    return array_frame(mp, a);
}

int sva_array_depth_mb(void* mp, const uint8_t* const* images, int n_images, int W, int H,
                       size_t pitch, const sva_array_pair* pairs, int n_pairs,
                       const int32_t* group_start, int n_groups, double f, double pixel_size,
                       int uniqueness, double* depth, uint16_t* maps, uint16_t* cost_min,
                       uint16_t* cost_second) {
    ArrayArgs a = frame_args(images, n_images, W, H, pitch, pairs, n_pairs, group_start, n_groups,
                             f, pixel_size, uniqueness, depth, maps, cost_min, cost_second);
    a.route = ArrayRoute::Groups;
    a.conf = true;
    return array_frame(mp, a);
}

int sva_array_depth_mixed(void* mp, const uint8_t* const* images, int n_images, int W, int H,
                          size_t pitch, const sva_array_pair* pairs, int n_pairs,
                          const int32_t* group_start, int n_groups, const double* unit_baseline,
                          double f, double pixel_size, int uniqueness, double* depth,
                          uint16_t* maps, uint16_t* cost_min, uint16_t* cost_second) {
    ArrayArgs a = frame_args(images, n_images, W, H, pitch, pairs, n_pairs, group_start, n_groups,
                             f, pixel_size, uniqueness, depth, maps, cost_min, cost_second);
    a.route = ArrayRoute::GroupsMixed;
    a.conf = true;
    a.unit_baseline = unit_baseline;
    return array_frame(mp, a);
}

int sva_array_depth_sub(void* mp, const uint8_t* const* images, int n_images, int W, int H,
                        size_t pitch, const sva_array_pair* pairs, int n_pairs,
                        const int32_t* group_start, int n_groups, int route,
                        const double* unit_baseline, double f, double pixel_size, int uniqueness,
                        int mode, double* depth, uint8_t* n_valid, uint8_t* winner, float* subpix,
                        uint16_t* maps, uint16_t* cost_min, uint16_t* cost_second) {
    ArrayArgs a = routed_args(images, n_images, W, H, pitch, pairs, n_pairs, group_start, n_groups,
                              route, unit_baseline, f, pixel_size, uniqueness, mode, depth, n_valid,
                              winner, subpix, maps, cost_min, cost_second);
    return sub_frame(mp, a, 1);
}

int sva_array_depth_checked(void* mp, const uint8_t* const* images, int n_images, int W, int H,
                            size_t pitch, const sva_array_pair* pairs, int n_pairs,
                            const int32_t* group_start, int n_groups, int route,
                            const double* unit_baseline, double f, double pixel_size,
                            int uniqueness, int mode, double* depth, uint8_t* n_valid,
                            uint8_t* winner, float* subpix, uint16_t* maps, uint16_t* cost_min,
                            uint16_t* cost_second, const int32_t* view_step, int sub, int max_diff,
                            int min_agree, int max_conflict, uint8_t* agree, uint8_t* conflict) {
    ArrayArgs a = routed_args(images, n_images, W, H, pitch, pairs, n_pairs, group_start, n_groups,
                              route, unit_baseline, f, pixel_size, uniqueness, mode, depth, n_valid,
                              winner, subpix, maps, cost_min, cost_second);
    set_cross(a, true, view_step, max_diff, min_agree, max_conflict, agree, conflict);
    return sub_frame(mp, a, sub);
}

// check = 0: the check's arguments are not looked at.
int sva_array_depth_filtered(void* mp, const uint8_t* const* images, int n_images, int W, int H,
                             size_t pitch, const sva_array_pair* pairs, int n_pairs,
                             const int32_t* group_start, int n_groups, int route,
                             const double* unit_baseline, double f, double pixel_size,
                             int uniqueness, int mode, double* depth, uint8_t* n_valid,
                             uint8_t* winner, float* subpix, uint16_t* maps, uint16_t* cost_min,
                             uint16_t* cost_second, const int32_t* view_step, int sub, int max_diff,
                             int min_agree, int max_conflict, uint8_t* agree, uint8_t* conflict,
                             int check, int speckle_max_size, int speckle_max_diff,
                             uint32_t* comp_size) {
    ArrayArgs a = routed_args(images, n_images, W, H, pitch, pairs, n_pairs, group_start, n_groups,
                              route, unit_baseline, f, pixel_size, uniqueness, mode, depth, n_valid,
                              winner, subpix, maps, cost_min, cost_second);
    set_cross(a, check == 1, view_step, max_diff, min_agree, max_conflict, agree, conflict);
    set_speckle(a, check, speckle_max_size, speckle_max_diff, comp_size);
    return sub_frame(mp, a, sub);
}

int sva_array_depth_filled(void* mp, const uint8_t* const* images, int n_images, int W, int H,
                           size_t pitch, const sva_array_pair* pairs, int n_pairs,
                           const int32_t* group_start, int n_groups, int route,
                           const double* unit_baseline, double f, double pixel_size, int uniqueness,
                           int mode, double* depth, uint8_t* n_valid, uint8_t* winner,
                           float* subpix, uint16_t* maps, uint16_t* cost_min, uint16_t* cost_second,
                           const int32_t* view_step, int sub, int max_diff, int min_agree,
                           int max_conflict, uint8_t* agree, uint8_t* conflict, int check,
                           int speckle_max_size, int speckle_max_diff, uint32_t* comp_size,
                           int fill_max_dist, int fill_min_found, int fill_mode, uint8_t* n_found) {
    ArrayArgs a = routed_args(images, n_images, W, H, pitch, pairs, n_pairs, group_start, n_groups,
                              route, unit_baseline, f, pixel_size, uniqueness, mode, depth, n_valid,
                              winner, subpix, maps, cost_min, cost_second);
    set_cross(a, check == 1, view_step, max_diff, min_agree, max_conflict, agree, conflict);
    set_speckle(a, check, speckle_max_size, speckle_max_diff, comp_size);
    set_fill(a, fill_max_dist, fill_min_found, fill_mode, n_found);
    return sub_frame(mp, a, sub);
}

int sva_array_depth_smoothed(void* mp, const uint8_t* const* images, int n_images, int W, int H,
                             size_t pitch, const sva_array_pair* pairs, int n_pairs,
                             const int32_t* group_start, int n_groups, int route,
                             const double* unit_baseline, double f, double pixel_size,
                             int uniqueness, int mode, double* depth, uint8_t* n_valid,
                             uint8_t* winner, float* subpix, uint16_t* maps, uint16_t* cost_min,
                             uint16_t* cost_second, const int32_t* view_step, int sub, int max_diff,
                             int min_agree, int max_conflict, uint8_t* agree, uint8_t* conflict,
                             int check, int speckle_max_size, int speckle_max_diff,
                             uint32_t* comp_size, int fill_max_dist, int fill_min_found,
                             int fill_mode, uint8_t* n_found, int wmed_radius,
                             const uint16_t* wmed_weights, int wmed_min_support, int wmed_select,
                             uint16_t* support) {
    ArrayArgs a = routed_args(images, n_images, W, H, pitch, pairs, n_pairs, group_start, n_groups,
                              route, unit_baseline, f, pixel_size, uniqueness, mode, depth, n_valid,
                              winner, subpix, maps, cost_min, cost_second);
    set_cross(a, check == 1, view_step, max_diff, min_agree, max_conflict, agree, conflict);
    set_speckle(a, check, speckle_max_size, speckle_max_diff, comp_size);
    set_fill(a, fill_max_dist, fill_min_found, fill_mode, n_found);
    set_wmed(a, wmed_radius, wmed_weights, wmed_min_support, wmed_select, support);
    return sub_frame(mp, a, sub);
}

// wmed_radius = 0: the weighted median is off (this entry only).
int sva_array_depth_rectified(void* mp, const uint8_t* const* images, int n_images, int W, int H,
                              size_t pitch, const sva_array_pair* pairs, int n_pairs,
                              const int32_t* group_start, int n_groups, int route,
                              const double* unit_baseline, double f, double pixel_size,
                              int uniqueness, int mode, double* depth, uint8_t* n_valid,
                              uint8_t* winner, float* subpix, uint16_t* maps, uint16_t* cost_min,
                              uint16_t* cost_second, const int32_t* view_step, int sub,
                              int max_diff, int min_agree, int max_conflict, uint8_t* agree,
                              uint8_t* conflict, int check, int speckle_max_size,
                              int speckle_max_diff, uint32_t* comp_size, int fill_max_dist,
                              int fill_min_found, int fill_mode, uint8_t* n_found, int wmed_radius,
                              const uint16_t* wmed_weights, int wmed_min_support, int wmed_select,
                              uint16_t* support, const sva_rectify_view* rect, int border,
                              int mask, uint8_t* views_out, uint8_t* valid_out) {
    ArrayArgs a = routed_args(images, n_images, W, H, pitch, pairs, n_pairs, group_start, n_groups,
                              route, unit_baseline, f, pixel_size, uniqueness, mode, depth, n_valid,
                              winner, subpix, maps, cost_min, cost_second);
    set_cross(a, check == 1, view_step, max_diff, min_agree, max_conflict, agree, conflict);
    set_speckle(a, check, speckle_max_size, speckle_max_diff, comp_size);
    set_fill(a, fill_max_dist, fill_min_found, fill_mode, n_found);
    set_wmed(a, wmed_radius, wmed_weights, wmed_min_support, wmed_select, support);
    a.wmed = wmed_radius != 0;
    if (!a.wmed) a.support = nullptr;   // no stage writes it: left untouched
    a.rect = true;
    a.rect_views = rect;
    a.rect_border = border;
    a.rect_mask = mask;
    a.views_out = views_out;
    a.valid_out = valid_out;
    return sub_frame(mp, a, sub);
}

}  // extern "C"
