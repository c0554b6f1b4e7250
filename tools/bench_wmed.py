#!/usr/bin/env python3
"""The weighted median filter: its launch against a copy
of the bytes its model says it moves, over radii, guided and unguided and
select shares, and the array route that runs it.

--kernel   1080p, n = 1 and 25 synthetic maps with 5 % holes and a random u8
           guide each.  On one warm context, 15 calls of sva_weighted_median_d in
           each case (3 more to warm up), timed by a pair of stream events around
           the call, next to a device copy that moves the bytes of the model --
           per pixel 2 read (+1 guided, +1 with select) and 2 written for the u16
           planes alone; +4 read, +6 written with out_sub and support -- timed the
           same way.  The copy goes round a ring of initialised buffers that
           together exceed 1 GiB, so no call finds its bytes in the 256 MB
           Infinity Cache: the column is HBM time.  Cases:
             radius   1, 2, 5, 7, 15, guided (sigma 32) and unguided, fill 1,
                      maps of values 1..100 at random ("noise": the bisection
                      takes its most steps)
             maps     r = 5 again on "smooth" maps (two planes 8 apart and +-1
                      noise: what a disparity map looks like to the bisection)
             select   r = 5 guided: a select plane with 5 % and 100 % of the
                      pixels lit at random, and one that lights 5 % of the tiles
                      (the others are skipped)
             planes   r = 5 guided with out_sub and support
--array    a center8-style frame at 1080p D = 128 on SVA_ARRAY_GROUPS with three
           reference cameras (11, 12, 13 of the 5x5 rig, eight neighbours each),
           check 1, speckle 20 / 1, fill 16 / 3 MEDIAN: sva_array_depth_filled,
           sva_array_depth_smoothed (r = 5, sigma 32) with wmed_select 0, with
           wmed_select 1, sva_array_depth_filled again (A-B-A in one session),
           host images in and depth out, `--steps` calls per phase.
Prints one JSON line per mode.  Reported, not asserted.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = 15
RADII = (1, 2, 5, 7, 15)
SIGMA = 32
RING_BYTES = 5 << 28           # the copy's ring: 1.25 GiB, five times the Infinity Cache
GRID5 = [(i % 5 - 2, i // 5 - 2) for i in range(25)]


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
            "max": round(max(v), 4), "n": len(v)}


def model_bytes(n, W, H, guided, select, full):
    per = 2 + (1 if guided else 0) + (1 if select else 0) + 2 + (10 if full else 0)
    return n * W * H * per


def kernel_mode(a, sva, W, H):
    import torch
    ctx = sva.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    weights = sva.wmed_weights(SIGMA)
    out = {"mode": "kernel", "size": f"{W}x{H}", "calls": CALLS, "sigma": SIGMA,
           "cases": []}

    def maps_of(n, kind, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        if kind == "noise":
            d = torch.randint(1, 101, (n, H, W), generator=g, device="cuda", dtype=torch.int16)
        else:
            d = torch.full((n, H, W), 20, device="cuda", dtype=torch.int16)
            d[:, H // 3:2 * H // 3, W // 3:2 * W // 3] = 28
            d += torch.randint(-1, 2, (n, H, W), generator=g, device="cuda", dtype=torch.int16)
        gone = torch.rand((n, H, W), generator=g, device="cuda") < 0.05
        d[gone] = -1
        guide = torch.randint(0, 256, (n, H, W), generator=g, device="cuda", dtype=torch.uint8)
        return d, d.to(torch.float32) + 0.25, guide

    def timed(n, d, s, guide, sel, r, o, os_, sup):
        gp = None if guide is None else [guide[k].data_ptr() for k in range(n)]

        def call():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            ctx.weighted_median_d(d.data_ptr(), None if s is None else s.data_ptr(), gp, W,
                                  None if guide is None else weights,
                                  None if sel is None else sel.data_ptr(), n, W, H, 0xFFFF, r, 1, 1,
                                  o.data_ptr(), None if os_ is None else os_.data_ptr(),
                                  None if sup is None else sup.data_ptr())
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        for _ in range(3):
            call()
        return [call() for _ in range(CALLS)]

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
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            dst.copy_(src)
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        for _ in range(pairs + 3):
            call()
        return [call() for _ in range(CALLS)]

    def case(n, d, s, guide, o, os_, sup, r, kind, guided, sel=None, sel_name=None, full=False):
        nbytes = model_bytes(n, W, H, guided, sel is not None, full)
        tc = copy_of(nbytes)
        t = timed(n, d, s if full else None, guide if guided else None, sel, r, o,
                  os_ if full else None, sup if full else None)
        out["cases"].append({
            "n": n, "radius": r, "maps": kind, "guided": guided, "select": sel_name,
            "planes": "u16+f32+support" if full else "u16", "model_bytes": nbytes,
            "wmed_ms": summary(t), "copy_ms": summary(tc),
            "wmed_over_copy": round(statistics.median(t) / statistics.median(tc), 2),
            "changed_pixels": int((o != d).sum())})

    for n in (1, 25):
        d, s, guide = maps_of(n, "noise", 11)
        o, os_ = torch.zeros_like(d), torch.zeros_like(s)
        sup = torch.zeros_like(d)
        for r in RADII:
            for guided in (True, False):
                case(n, d, s, guide, o, os_, sup, r, "noise", guided)
        g = torch.Generator(device="cuda").manual_seed(5)
        lit5 = (torch.rand(d.shape, generator=g, device="cuda") < 0.05).to(torch.uint8)
        tiles5 = (torch.rand((n, (H + 7) // 8, (W + 31) // 32), generator=g, device="cuda") < 0.05)
        tiles5 = tiles5.repeat_interleave(8, 1).repeat_interleave(32, 2)[:, :H, :W]
        for name, sel in (("5% of pixels", lit5), ("100%", torch.ones_like(lit5)),
                          ("5% of 32x8 tiles", tiles5.to(torch.uint8).contiguous())):
            case(n, d, s, guide, o, os_, sup, 5, "noise", True, sel, name)
        case(n, d, s, guide, o, os_, sup, 5, "noise", True, full=True)
        del d, s, guide
        d, s, guide = maps_of(n, "smooth", 12)
        for guided in (True, False):
            case(n, d, s, guide, o, os_, sup, 5, "smooth", guided)
        del d, s, guide, o, os_, sup
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
    post = dict(speckle_max_size=20, speckle_max_diff=1, check=1, view_step=steps, max_diff=1,
                min_agree=2, max_conflict=8)
    weights = sva.wmed_weights(SIGMA)
    m = sva.Multi([0], streams=a.streams)

    def filled():
        return m.array_depth_filled(views, jobs, gs, f, ps, 16, 3, sva.SVA_FILL_MEDIAN, **post)

    def smoothed(select):
        return m.array_depth_smoothed(views, jobs, gs, f, ps, 5, weights, 1, select,
                                      fill_max_dist=16, fill_min_found=3,
                                      fill_mode=sva.SVA_FILL_MEDIAN, **post)

    routes = {"filled": filled, "smoothed": lambda: smoothed(0), "smoothed_select": lambda: smoothed(1)}
    try:
        for _ in range(a.warmup):
            for r in routes.values():
                r()
        timed = []
        for name in ("filled", "smoothed", "smoothed_select", "filled"):
            v = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                routes[name]()
                v.append((time.perf_counter() - t0) * 1e3)
            timed.append((name, v))
        c0 = m.context(0, 0)
        c0.set_timing(sva.SVA_TIMING_ALL)
        k_ms = {}
        for name, sel in (("smoothed", 0), ("smoothed_select", 1)):
            c0.reset_timing()
            smoothed(sel)
            k_ms[name] = round(c0.kernel_time("wmed")[0], 4)
        c0.set_timing(0)
    finally:
        m.close()
    by = {}
    for name, v in timed:
        by.setdefault(name, []).extend(v)
    med = lambda k: statistics.median(by[k])
    print(json.dumps({
        "mode": "array", "size": f"{W}x{H}", "D": a.D, "groups": 3, "pairs": len(jobs),
        "streams": a.streams, "steps_per_phase": a.steps, "radius": 5, "sigma": SIGMA,
        "phases": [{"route": n, "ms_per_call": summary(v)} for n, v in timed],
        "ms_per_call": {n: summary(v) for n, v in by.items()},
        "smoothed_minus_filled_ms": round(med("smoothed") - med("filled"), 4),
        "smoothed_select_minus_filled_ms": round(med("smoothed_select") - med("filled"), 4),
        "wmed_kernel_ms": k_ms}), flush=True)


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
        raise SystemExit("bench_wmed: no HIP device visible")
    if a.kernel:
        kernel_mode(a, sva, W, H)
    if a.array:
        array_mode(a, sva, synth, W, H)


if __name__ == "__main__":
    main()
