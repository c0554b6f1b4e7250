#!/usr/bin/env python3
"""The speckle filter: its four launches against a copy
of the bytes it has to move, and the array route that runs it.

--kernel   1080p, the maps of n = 1, 8 and 25 reference cameras of a 5x5 rig,
           each matched multi-baseline against its neighbours one grid unit away
           on views from synth.array_views (real maps: the components of random
           ones would all be a few pixels).  On one warm context, 15 calls of
           sva_filter_speckles_d (max_size 20, max_diff 1), then a plain device
           copy of the compulsory bytes on the same buffers (maps and f32 planes
           copied, comp_size filled).  Both are timed by a pair of stream events
           around the call, so the ratio compares like with like, launch gaps on
           both sides; the context's own kernel timer gives the four launches one
           by one.  Median and min-max of each, the filter's ratio to the copy,
           and which launch dominates.  Three plane sets: the u16 maps alone (4
           bytes per map and pixel), with the f32 planes (12), with comp_size too
           (16).
--array    a center8-style frame at 1080p D = 128 on SVA_ARRAY_GROUPS with three
           reference cameras (11, 12, 13 of the 5x5 rig, eight neighbours each):
           sva_array_depth_checked, sva_array_depth_filtered (check 1),
           sva_array_depth_checked again (A-B-A in one session), host images in
           and depth out, `--steps` calls per phase.  Reported, not asserted.
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
LAUNCHES = ("speckle_label", "speckle_merge", "speckle_count", "speckle_apply")
MAX_SIZE, MAX_DIFF = 20, 1


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
    views, jobs, gs = frame(sva, synth, list(range(25)), W, H, a.D)
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
           "max_size": MAX_SIZE, "max_diff": MAX_DIFF, "cases": []}
    for n in (1, 8, 25):
        refs = [12] if n == 1 else list(range(n))
        d = torch.from_numpy(np.ascontiguousarray(maps25[refs]).view(np.int16)).cuda()
        s = torch.from_numpy(np.ascontiguousarray(sub25[refs])).cuda()
        o, os_ = torch.zeros_like(d), torch.zeros_like(s)
        size = torch.zeros(d.shape, dtype=torch.int32, device="cuda")
        for planes, per_px in (("u16", 4), ("u16+f32", 12), ("u16+f32+size", 16)):
            with_sub, with_size = planes != "u16", planes.endswith("size")

            def call():
                ctx.reset_timing()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                ctx.filter_speckles_d(d.data_ptr(), s.data_ptr() if with_sub else None, n, W, H,
                                      0xFFFF, MAX_SIZE, MAX_DIFF, o.data_ptr(),
                                      os_.data_ptr() if with_sub else None,
                                      size.data_ptr() if with_size else None)
                e1.record(stream)
                e1.synchronize()
                each = {}
                for name in LAUNCHES:
                    ms, cnt = ctx.kernel_time(name)
                    assert cnt == 1
                    each[name] = ms
                return e0.elapsed_time(e1), each

            for _ in range(3):
                call()
            t, kt = [], {name: [] for name in LAUNCHES}
            for _ in range(CALLS):
                ev, each = call()
                t.append(ev)
                for name in LAUNCHES:
                    kt[name].append(each[name])

            def copy():
                o.copy_(d)
                if with_sub:
                    os_.copy_(s)
                if with_size:
                    size.fill_(1)

            removed = int(((o == -1) & (d != -1)).sum())
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
            med = {name: statistics.median(v) for name, v in kt.items()}
            out["cases"].append({
                "n": n, "planes": planes, "compulsory_bytes": n * W * H * per_px,
                "workspace_bytes": 8 * n * W * H, "filter_ms": summary(t), "copy_ms": summary(tc),
                "filter_over_copy": round(statistics.median(t) / statistics.median(tc), 2),
                "kernel_timer_ms": {name: summary(v) for name, v in kt.items()},
                "dominant_launch": max(med, key=med.get), "removed_pixels": removed})
    ctx.close()
    print(json.dumps(out), flush=True)


def array_mode(a, sva, synth, W, H):
    views, jobs, gs = frame(sva, synth, [11, 12, 13], W, H, a.D)
    steps = [(-gx, -gy) for gx, gy in GRID5]
    f, ps = 0.05, 0.036 / W
    check = dict(max_diff=1, min_agree=2, max_conflict=8)
    m = sva.Multi([0], streams=a.streams)

    def checked():
        return m.array_depth_checked(views, jobs, gs, f, ps, steps, uniqueness=a.uniqueness, **check)

    def filtered():
        return m.array_depth_filtered(views, jobs, gs, f, ps, MAX_SIZE, MAX_DIFF, check=1,
                                      view_step=steps, uniqueness=a.uniqueness, **check)

    routes = {"checked": checked, "filtered": filtered}
    try:
        for _ in range(a.warmup):
            checked(), filtered()
        timed = []
        for name in ("checked", "filtered", "checked"):
            v = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                routes[name]()
                v.append((time.perf_counter() - t0) * 1e3)
            timed.append((name, v))
        c0 = m.context(0, 0)
        c0.set_timing(sva.SVA_TIMING_ALL)
        c0.reset_timing()
        filtered()
        k_ms = {name: round(c0.kernel_time(name)[0], 4) for name in LAUNCHES}
        c0.set_timing(0)
    finally:
        m.close()
    by = {}
    for name, v in timed:
        by.setdefault(name, []).extend(v)
    print(json.dumps({
        "mode": "array", "size": f"{W}x{H}", "D": a.D, "groups": 3, "pairs": len(jobs),
        "streams": a.streams, "steps_per_phase": a.steps, "max_size": MAX_SIZE,
        "max_diff": MAX_DIFF,
        "phases": [{"route": n, "ms_per_call": summary(v)} for n, v in timed],
        "ms_per_call": {n: summary(v) for n, v in by.items()},
        "filtered_minus_checked_ms": round(statistics.median(by["filtered"]) -
                                           statistics.median(by["checked"]), 4),
        "speckle_kernel_ms": k_ms}), flush=True)


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
        raise SystemExit("bench_speckle: no HIP device visible")
    if a.kernel:
        kernel_mode(a, sva, synth, W, H)
    if a.array:
        array_mode(a, sva, synth, W, H)


if __name__ == "__main__":
    main()
