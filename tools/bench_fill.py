#!/usr/bin/env python3
"""Hole filling: its two launches against a copy of the
bytes its model says it moves, over hole shares, segment lengths and distances,
and the array route that runs it.

--kernel   1080p, n = 1 and 25 synthetic maps (values 1..100, a share of the
           pixels holes at random: the kernels' work depends on the map only
           through the hole share, which is what is varied).  On one warm
           context, 15 calls of sva_fill_holes_d in each case, timed by a pair of
           stream events around the call, next to a plain device copy that moves
           the same number of bytes as the model of §4.23 -- scan: 16 read, 32
           written per pixel; apply: 2 + 32 * share read, 2 written -- timed the
           same way.  The context's kernel timer gives the two launches one by
           one.  Cases:
             shares   5 %, 50 %, 100 %, then 5 % again (A-B-A: the spread of the
                      two 5 % legs is the margin the shares are compared with)
             planes   the u16 maps alone, and with the f32 planes and n_found
             sweep    kFillSegment in {8, 16, 32, 64, 128} (SVA_DEBUG_FILL_SEGMENT)
                      x max_dist in {16, 64, 255}, n = 25, 5 % holes
--array    a center8-style frame at 1080p D = 128 on SVA_ARRAY_GROUPS with three
           reference cameras (11, 12, 13 of the 5x5 rig, eight neighbours each),
           check 1, speckle 20 / 1: sva_array_depth_filtered, sva_array_depth_filled
           with max_dist 16, with max_dist 0, sva_array_depth_filtered again
           (A-B-A in one session), host images in and depth out, `--steps` calls
           per phase.  Reported, not asserted.
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
LAUNCHES = ("fill_scan", "fill_apply")
MAX_SIZE, MAX_DIFF = 20, 1
MAX_DIST, MIN_FOUND = 16, 3


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


def model_bytes(n, W, H, share):
    return int(n * W * H * (16 + 32 + 2 + 32 * share + 2))


def kernel_mode(a, sva, W, H):
    import torch
    ctx = sva.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    ctx.set_timing(sva.SVA_TIMING_ALL)
    mode = sva.SVA_FILL_MEDIAN
    out = {"mode": "kernel", "size": f"{W}x{H}", "calls": CALLS, "min_found": MIN_FOUND,
           "fill_mode": mode, "segment": ctx.get_debug(sva.SVA_DEBUG_FILL_SEGMENT), "cases": [],
           "sweep": []}

    def maps_of(n, share, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        d = torch.randint(1, 101, (n, H, W), generator=g, device="cuda", dtype=torch.int16)
        gone = torch.rand((n, H, W), generator=g, device="cuda") < share
        d[gone] = -1
        return d, d.to(torch.float32) + 0.25

    def timed(n, d, s, o, os_, found, max_dist):
        def call():
            ctx.reset_timing()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            ctx.fill_holes_d(d.data_ptr(), None if s is None else s.data_ptr(), n, W, H, 0xFFFF,
                             max_dist, MIN_FOUND, mode, o.data_ptr(),
                             None if os_ is None else os_.data_ptr(),
                             None if found is None else found.data_ptr())
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
        return t, kt

    def copy_of(nbytes):
        """A device copy that reads nbytes / 2 and writes nbytes / 2."""
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        for _ in range(3):
            dst.copy_(src)
        tc = []
        for _ in range(CALLS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            dst.copy_(src)
            e1.record(stream)
            e1.synchronize()
            tc.append(e0.elapsed_time(e1))
        return tc

    for n in (1, 25):
        for leg, share in enumerate((0.05, 0.5, 1.0, 0.05)):
            d, s = maps_of(n, share, 11)
            o, os_ = torch.zeros_like(d), torch.zeros_like(s)
            found = torch.zeros(d.shape, dtype=torch.uint8, device="cuda")
            tc = copy_of(model_bytes(n, W, H, share))
            for planes in ("u16", "u16+f32+found"):
                full = planes != "u16"
                t, kt = timed(n, d, s if full else None, o, os_ if full else None,
                              found if full else None, MAX_DIST)
                filled = int(((o != -1) & (d == -1)).sum())
                out["cases"].append({
                    "n": n, "hole_share": share, "leg": leg, "planes": planes, "max_dist": MAX_DIST,
                    "model_bytes": model_bytes(n, W, H, share), "workspace_bytes": 32 * n * W * H,
                    "fill_ms": summary(t), "copy_ms": summary(tc),
                    "fill_over_copy": round(statistics.median(t) / statistics.median(tc), 2),
                    "kernel_timer_ms": {name: summary(v) for name, v in kt.items()},
                    "holes": int((d == -1).sum()), "filled_pixels": filled})
            del d, s, o, os_, found
    n = 25
    d, _ = maps_of(n, 0.05, 11)
    o = torch.zeros_like(d)
    try:
        for seg in (8, 16, 32, 64, 128):
            ctx.set_debug(sva.SVA_DEBUG_FILL_SEGMENT, seg)
            for md in (16, 64, 255):
                t, kt = timed(n, d, None, o, None, None, md)
                out["sweep"].append({"n": n, "hole_share": 0.05, "segment": seg, "max_dist": md,
                                     "fill_ms": summary(t),
                                     "kernel_timer_ms": {k: summary(v) for k, v in kt.items()}})
    finally:
        ctx.set_debug(sva.SVA_DEBUG_FILL_SEGMENT, 0)
    ctx.close()
    print(json.dumps(out), flush=True)


def array_mode(a, sva, synth, W, H):
    views, jobs, gs = frame(sva, synth, [11, 12, 13], W, H, a.D)
    steps = [(-gx, -gy) for gx, gy in GRID5]
    f, ps = 0.05, 0.036 / W
    check = dict(max_diff=1, min_agree=2, max_conflict=8)
    m = sva.Multi([0], streams=a.streams)

    def filtered():
        return m.array_depth_filtered(views, jobs, gs, f, ps, MAX_SIZE, MAX_DIFF, check=1,
                                      view_step=steps, uniqueness=a.uniqueness, **check)

    def filled(max_dist):
        return m.array_depth_filled(views, jobs, gs, f, ps, max_dist, MIN_FOUND,
                                    sva.SVA_FILL_MEDIAN, speckle_max_size=MAX_SIZE,
                                    speckle_max_diff=MAX_DIFF, check=1, view_step=steps,
                                    uniqueness=a.uniqueness, **check)

    routes = {"filtered": filtered, "filled": lambda: filled(MAX_DIST), "filled_0": lambda: filled(0)}
    try:
        for _ in range(a.warmup):
            for r in routes.values():
                r()
        timed = []
        for name in ("filtered", "filled", "filled_0", "filtered"):
            v = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                routes[name]()
                v.append((time.perf_counter() - t0) * 1e3)
            timed.append((name, v))
        c0 = m.context(0, 0)
        c0.set_timing(sva.SVA_TIMING_ALL)
        c0.reset_timing()
        filled(MAX_DIST)
        k_ms = {name: round(c0.kernel_time(name)[0], 4) for name in LAUNCHES}
        c0.set_timing(0)
    finally:
        m.close()
    by = {}
    for name, v in timed:
        by.setdefault(name, []).extend(v)
    med = lambda k: statistics.median(by[k])
    print(json.dumps({
        "mode": "array", "size": f"{W}x{H}", "D": a.D, "groups": 3, "pairs": len(jobs),
        "streams": a.streams, "steps_per_phase": a.steps, "max_dist": MAX_DIST,
        "min_found": MIN_FOUND,
        "phases": [{"route": n, "ms_per_call": summary(v)} for n, v in timed],
        "ms_per_call": {n: summary(v) for n, v in by.items()},
        "filled_minus_filtered_ms": round(med("filled") - med("filtered"), 4),
        "filled_0_minus_filtered_ms": round(med("filled_0") - med("filtered"), 4),
        "fill_kernel_ms": k_ms}), flush=True)


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
        raise SystemExit("bench_fill: no HIP device visible")
    if a.kernel:
        kernel_mode(a, sva, W, H)
    if a.array:
        array_mode(a, sva, synth, W, H)


if __name__ == "__main__":
    main()
