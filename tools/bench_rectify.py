#!/usr/bin/env python3
"""Rectification: its launch against a copy of the bytes
its model says it moves, and the array frame that runs it.

--kernel   1080p in and out, n = 1, 9 and 25 random u8 views.  On one warm
           context, 15 calls of sva_rectify_d in each case (3 more to warm up),
           timed by a pair of stream events around the call, next to a device
           copy that moves the bytes of the model -- per pixel and view 1 read
           (the source) and 1 written, +1 written with the valid plane -- timed the
           same way on a ring of initialised buffers that together exceed 1 GiB,
           so that no call finds its bytes in the 256 MB Infinity Cache.  Models:
             plain    h = a 2.5 px shift: no distortion step, w = 1
             affine   a 0.7 degree roll and a shift, no distortion step
             full     roll, shift, perspective terms, k1 k2 p1 p2 k3
           each without and with the valid plane; `full` also with the map.
--array    a center8-style frame at 1080p D = 128 on SVA_ARRAY_GROUPS with three
           reference cameras (11, 12, 13 of the 5x5 rig, eight neighbours each),
           check 1, speckle 20 / 1, fill 16 / 3 MEDIAN, median r = 5 sigma 32:
           sva_array_depth_smoothed, sva_array_depth_rectified with the `full`
           model per view and mask 1 on the same views, sva_array_depth_smoothed
           again (A-B-A in one session, one engine), host images in and depth
           out, `--steps` calls per phase.
Prints one JSON line per mode.  Reported, not asserted.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = 15
SIGMA = 32
RING_BYTES = 5 << 28           # the copy's ring: 1.25 GiB, five times the Infinity Cache
GRID5 = [(i % 5 - 2, i // 5 - 2) for i in range(25)]


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
            "max": round(max(v), 4), "n": len(v)}


def model(sva, kind, W, H, i=0):
    """View i's model of a kind: plain, affine or full."""
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    if kind == "plain":
        return sva.RectifyView.make((1, 0, 2.5, 0, 1, -1.5, 0, 0, 1))
    t = math.radians(0.7 - 0.05 * (i % 9))
    c, s = math.cos(t), math.sin(t)
    h = [c, -s, cx - c * cx + s * cy + 2.0, s, c, cy - s * cx - c * cy - 1.5, 0, 0, 1]
    if kind == "affine":
        return sva.RectifyView.make(h)
    h[6], h[7] = 2e-6, -1e-6
    return sva.RectifyView.make(h, cx, cy, float(W), float(W), (-0.12, 0.03, 1e-3, -2e-3, 0.01))


def kernel_mode(a, sva, W, H):
    import torch
    ctx = sva.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    out = {"mode": "kernel", "size": f"{W}x{H}", "calls": CALLS, "cases": []}

    def timed(call):
        def once():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)
        return once

    def copy_of(nbytes):
        """A device copy that reads nbytes / 2 and writes nbytes / 2, each call on
        the next pair of a ring of initialised buffers larger than the cache."""
        half = nbytes // 2
        pairs = max(2, -(-RING_BYTES // nbytes))
        ring = [(torch.full((half,), 3, dtype=torch.uint8, device="cuda"),
                 torch.zeros(half, dtype=torch.uint8, device="cuda")) for _ in range(pairs)]
        turn = [0]

        def call():
            src, dst = ring[turn[0] % pairs]
            turn[0] += 1
            dst.copy_(src)

        once = timed(call)
        for _ in range(pairs + 3):
            once()
        return [once() for _ in range(CALLS)]

    for n in (1, 9, 25):
        g = torch.Generator(device="cuda").manual_seed(3)
        src = torch.randint(0, 256, (n, H, W), generator=g, device="cuda", dtype=torch.uint8)
        dst, valid = torch.zeros_like(src), torch.zeros_like(src)
        qmap = torch.zeros((n, H, W, 2), device="cuda", dtype=torch.int32)
        # the model's bytes: with valid 1.5 times a plain copy's; the copy stays a
        # read-half write-half copy of that many bytes
        copies = {planes: copy_of(n * W * H * planes) for planes in (2, 3)}
        for kind in ("plain", "affine", "full"):
            # the C table once, so that a call is the launch and nothing else
            rect = sva._view_table([model(sva, kind, W, H, i) for i in range(n)])
            for planes in ("out", "out+valid", "out+valid+map"):
                if planes == "out+valid+map" and kind != "full":
                    continue
                v = valid.data_ptr() if planes != "out" else None
                q = qmap.data_ptr() if planes == "out+valid+map" else None
                once = timed(lambda: ctx.rectify_d(src.data_ptr(), n, W, H, W, rect, W, H, W, 0,
                                                   dst.data_ptr(), v, q))
                for _ in range(3):
                    once()
                t = [once() for _ in range(CALLS)]
                tc = copies[2 if planes == "out" else 3]
                out["cases"].append({
                    "n": n, "model": kind, "planes": planes,
                    "model_bytes": n * W * H * (2 if planes == "out" else 3),
                    "rectify_ms": summary(t), "copy_ms": summary(tc),
                    "rectify_over_copy": round(statistics.median(t) / statistics.median(tc), 2),
                    "valid_share": round(float((valid != 0).float().mean()), 4) if v else None})
        del src, dst, valid, qmap, copies
    ctx.close()
    print(json.dumps(out), flush=True)


def neighbours(r):
    return [j for j in range(25) if j != r and
            max(abs(GRID5[j][0] - GRID5[r][0]), abs(GRID5[j][1] - GRID5[r][1])) == 1]


def array_mode(a, sva, synth, W, H):
    delta = synth.array_delta(H, W, min(a.D - 1, 100))
    views = synth.array_views(H, W, GRID5, delta, seed=7)
    jobs, gs = [], [0]
    for r in (11, 12, 13):
        for j in neighbours(r):
            sx, sy, k = synth.pair_step(GRID5[r], GRID5[j])
            jobs.append((r, j, sva.default_params(D=a.D, dir=sx, dir_y=sy), k * 0.05))
        gs.append(len(jobs))
    steps = [(-gx, -gy) for gx, gy in GRID5]
    f, ps = 0.05, 0.036 / W
    chain = dict(wmed_radius=5, wmed_weights=sva.wmed_weights(SIGMA), wmed_min_support=1,
                 wmed_select=0, fill_max_dist=16, fill_min_found=3, fill_mode=sva.SVA_FILL_MEDIAN,
                 speckle_max_size=20, speckle_max_diff=1, check=1, view_step=steps, max_diff=1,
                 min_agree=2, max_conflict=8)
    rect = [model(sva, "full", W, H, i) for i in range(25)]
    m = sva.Multi([0], streams=a.streams)
    routes = {
        "smoothed": lambda: m.array_depth_smoothed(views, jobs, gs, f, ps, **chain),
        "rectified": lambda: m.array_depth_rectified(views, rect, jobs, gs, f, ps, mask=1, **chain)}
    try:
        for _ in range(a.warmup):
            for r in routes.values():
                r()
        timed = []
        for name in ("smoothed", "rectified", "smoothed"):
            v = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                routes[name]()
                v.append((time.perf_counter() - t0) * 1e3)
            timed.append((name, v))
        c0 = m.context(0, 0)
        c0.set_timing(sva.SVA_TIMING_ALL)
        c0.reset_timing()
        routes["rectified"]()
        k_ms = {k: round(c0.kernel_time(k)[0], 4) for k in ("rectify", "mask_maps")}
        k_n = {k: c0.kernel_time(k)[1] for k in ("rectify", "mask_maps")}
        c0.set_timing(0)
    finally:
        m.close()
    by = {}
    for name, v in timed:
        by.setdefault(name, []).extend(v)
    med = lambda k: statistics.median(by[k])
    print(json.dumps({
        "mode": "array", "size": f"{W}x{H}", "D": a.D, "groups": 3, "pairs": len(jobs),
        "views_rectified": 15, "streams": a.streams, "steps_per_phase": a.steps,
        "phases": [{"route": n, "ms_per_call": summary(v)} for n, v in timed],
        "ms_per_call": {n: summary(v) for n, v in by.items()},
        "rectified_minus_smoothed_ms": round(med("rectified") - med("smoothed"), 4),
        "kernel_ms": k_ms, "kernel_calls": k_n}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--array", action="store_true")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--D", type=int, default=128)
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
        raise SystemExit("bench_rectify: no HIP device visible")
    if a.kernel:
        kernel_mode(a, sva, W, H)
    if a.array:
        array_mode(a, sva, synth, W, H)


if __name__ == "__main__":
    main()
