#!/usr/bin/env python3
"""The cross-view consistency check: its kernel against
a copy of the bytes it has to move, and the array route that runs it.

--kernel   1080p, the maps of n = 9 (the inner 3x3) and n = 25 reference cameras
           of a 5x5 rig, each matched multi-baseline against its neighbours one
           grid unit away on views from synth.array_views (real maps: random
           ones would have none of the locality the gathers rely on).  On one
           warm context the two block orders of cross_check alternate call by
           call, 15 calls each, with the outputs asserted equal; then a plain
           device copy of the compulsory bytes on the same buffers (maps and
           f32 planes copied, the count planes filled: up to four launches).
           Both are timed by a pair of stream events around the call, so the
           ratio compares like with like, launch gaps on both sides; the
           context's own kernel timer is reported next to it.  Median and
           min-max of each, and the kernel's ratio to the copy.  Twice: with
           every plane (14 bytes per view and pixel), and with the u16 maps
           alone (4).
--array    a center8-style frame at 1080p D = 128 on SVA_ARRAY_GROUPS with three
           reference cameras (11, 12, 13 of the 5x5 rig, eight neighbours each):
           sva_array_depth_mb, sva_array_depth_checked, sva_array_depth_mb again
           (A-B-A in one session), host images in and depth out, `--steps` calls
           per phase.  The difference is the kernel plus the download of the two
           count planes; it is reported, not asserted.
Prints one JSON line per mode.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID5 = [(i % 5 - 2, i // 5 - 2) for i in range(25)]
CALLS = 15


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
            "max": round(max(v), 4), "n": len(v)}


def neighbours(r):
    return [j for j in range(25) if j != r and
            max(abs(GRID5[j][0] - GRID5[r][0]), abs(GRID5[j][1] - GRID5[r][1])) == 1]


def frame(sva, synth, refs, W, H, D):
    """(views, jobs, group_start) of the reference cameras `refs` of the 5x5 rig."""
    delta = synth.array_delta(H, W, min(D - 1, 100))
    views = synth.array_views(H, W, GRID5, delta, seed=7)
    jobs, gs = [], [0]
    for r in refs:
        for j in neighbours(r):
            sx, sy, k = synth.pair_step(GRID5[r], GRID5[j])
            jobs.append((r, j, sva.default_params(D=D, dir=sx, dir_y=sy), k * 0.05))
        gs.append(len(jobs))
    return views, jobs, gs


def kernel_mode(a, sva, synth, W, H):
    import numpy as np
    import torch
    refs25 = list(range(25))
    views, jobs, gs = frame(sva, synth, refs25, W, H, a.D)
    m = sva.Multi([0], streams=2)
    try:
        res = m.array_depth_sub(views, jobs, gs, 0.05, 0.036 / W, route=sva.SVA_ARRAY_GROUPS,
                                uniqueness=a.uniqueness, want_sub=True, want_maps=True)
    finally:
        m.close()
    maps25, sub25 = res[4], res[3]
    ctx = sva.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    ctx.set_timing(sva.SVA_TIMING_ALL)
    out = {"mode": "kernel", "size": f"{W}x{H}", "D": a.D, "calls": CALLS,
           "thresholds": {"max_diff": 1, "min_agree": 2, "max_conflict": 8}, "cases": []}
    inner = [r for r in refs25 if max(abs(GRID5[r][0]), abs(GRID5[r][1])) <= 1]
    for refs in (inner, refs25):
        n = len(refs)
        steps = [(-GRID5[r][0], -GRID5[r][1]) for r in refs]
        d = torch.from_numpy(np.ascontiguousarray(maps25[refs]).view(np.int16)).cuda()
        s = torch.from_numpy(np.ascontiguousarray(sub25[refs])).cuda()
        o = [torch.zeros_like(d) for _ in range(2)]
        os_ = [torch.zeros_like(s) for _ in range(2)]
        ag = [torch.zeros(d.shape, dtype=torch.uint8, device="cuda") for _ in range(2)]
        cf = [torch.zeros(d.shape, dtype=torch.uint8, device="cuda") for _ in range(2)]
        for planes in ("all", "u16"):
            full = planes == "all"

            def call(order):
                ctx.set_debug(sva.SVA_DEBUG_CROSS_ORDER, order)
                ctx.reset_timing()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                ctx.cross_check_d(d.data_ptr(), s.data_ptr() if full else None, n, W, H, steps,
                                  0xFFFF, 1, 2, 8, o[order].data_ptr(),
                                  os_[order].data_ptr() if full else None,
                                  ag[order].data_ptr() if full else None,
                                  cf[order].data_ptr() if full else None)
                e1.record(stream)
                e1.synchronize()
                ms, cnt = ctx.kernel_time("cross_check")
                assert cnt == 1
                return e0.elapsed_time(e1), ms

            for _ in range(3):
                call(0), call(1)
            t, kt = {0: [], 1: []}, {0: [], 1: []}
            for _ in range(CALLS):
                for order in (0, 1):
                    ev, ms = call(order)
                    t[order].append(ev)
                    kt[order].append(ms)
                assert torch.equal(o[0], o[1])
                if full:
                    assert torch.equal(ag[0], ag[1]) and torch.equal(cf[0], cf[1])
                    assert torch.equal(os_[0].view(torch.int32), os_[1].view(torch.int32))
            ctx.set_debug(sva.SVA_DEBUG_CROSS_ORDER, -1)

            def copy():
                o[0].copy_(d)
                if full:
                    os_[0].copy_(s)
                    ag[0].fill_(1)
                    cf[0].fill_(1)

            for _ in range(3):
                copy()
            tc = []
            for _ in range(CALLS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                copy()
                e1.record(stream)
                e1.synchronize()
                tc.append(e0.elapsed_time(e1))
            per_px = 14 if full else 4
            rejected = int(((o[0] == -1) & (d != -1)).sum())
            case = {"n": n, "planes": planes, "compulsory_bytes": n * W * H * per_px,
                    "gather_bytes": n * (n - 1) * W * H * 2,
                    "view_major_ms": summary(t[0]), "tile_major_ms": summary(t[1]),
                    "view_major_kernel_timer_ms": summary(kt[0]),
                    "tile_major_kernel_timer_ms": summary(kt[1]),
                    "copy_ms": summary(tc), "rejected_pixels": rejected}
            med = {k: statistics.median(v) for k, v in (("v", t[0]), ("t", t[1]), ("c", tc))}
            case["view_major_over_copy"] = round(med["v"] / med["c"], 2)
            case["tile_major_over_copy"] = round(med["t"] / med["c"], 2)
            # outside both spreads: one order's slowest call beats the other's fastest
            case["tile_major_wins_outside_spreads"] = max(t[1]) < min(t[0])
            case["view_major_wins_outside_spreads"] = max(t[0]) < min(t[1])
            out["cases"].append(case)
    ctx.close()
    print(json.dumps(out), flush=True)


def array_mode(a, sva, synth, W, H):
    views, jobs, gs = frame(sva, synth, [11, 12, 13], W, H, a.D)
    steps = [(-gx, -gy) for gx, gy in GRID5]
    f, ps = 0.05, 0.036 / W
    m = sva.Multi([0], streams=a.streams)

    def mb():
        return m.array_depth_mb(views, jobs, gs, f, ps, a.uniqueness)

    def checked():
        return m.array_depth_checked(views, jobs, gs, f, ps, steps, uniqueness=a.uniqueness,
                                     max_diff=1, min_agree=2, max_conflict=8, want_counts=True)

    routes = {"mb": mb, "checked": checked}
    try:
        for _ in range(a.warmup):
            mb(), checked()
        timed = []
        for name in ("mb", "checked", "mb"):
            v = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                routes[name]()
                v.append((time.perf_counter() - t0) * 1e3)
            timed.append((name, v))
        c0 = m.context(0, 0)
        c0.set_timing(sva.SVA_TIMING_ALL)
        c0.reset_timing()
        checked()
        k_ms = c0.kernel_time("cross_check")[0]
        c0.set_timing(0)
    finally:
        m.close()
    by = {}
    for name, v in timed:
        by.setdefault(name, []).extend(v)
    print(json.dumps({
        "mode": "array", "size": f"{W}x{H}", "D": a.D, "groups": 3, "pairs": len(jobs),
        "streams": a.streams, "steps_per_phase": a.steps,
        "phases": [{"route": n, "ms_per_call": summary(v)} for n, v in timed],
        "ms_per_call": {n: summary(v) for n, v in by.items()},
        "checked_minus_mb_ms": round(statistics.median(by["checked"]) -
                                     statistics.median(by["mb"]), 4),
        "cross_check_kernel_ms": round(k_ms, 4),
        "count_planes_bytes": 2 * 3 * W * H}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--array", action="store_true")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--uniqueness", type=int, default=0)
    ap.add_argument("--steps", type=int, default=10, help="--array: calls per phase")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--streams", type=int, default=3)
    a = ap.parse_args()
    if not (a.kernel or a.array):
        ap.error("give --kernel and / or --array")
    W, H = map(int, a.size.split("x"))
    import stereovisionarray_amd as sva
    from stereovisionarray_amd import synth
    if sva.device_count() < 1:
        raise SystemExit("bench_cross_check: no HIP device visible")
    if a.kernel:
        kernel_mode(a, sva, synth, W, H)
    if a.array:
        array_mode(a, sva, synth, W, H)


if __name__ == "__main__":
    main()
