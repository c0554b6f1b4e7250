#!/usr/bin/env python3
"""What sub-pixel depth costs, in the manner of tools/bench_conf.py.

Kernels (default): on device planes of --size, for every n of --maps, the event
timers (SVA_TIMING_ALL) of
  fuse_depth           sva_fuse_depth_d
  fuse_depth_sub       sva_fuse_depth_sub_d
  fuse_depth_conf      sva_fuse_depth_conf_d, SVA_FUSE_MAX_MARGIN (both cost planes)
  fuse_depth_conf_sub  sva_fuse_depth_conf_sub_d, the same mode
run round-robin, ms per launch (median, min, max of --steps) and the bytes each
launch moves over that median: 2 n + 9 per pixel for the median (6 n + 9 with the
f32 planes), 6 n + 10 for the cost-aware form (10 n + 10).

--array: the center8 frame (camera 12 of a 5x5 grid against its eight
neighbours) at --size and --D, host images in, depth out, on an engine of one
device and three streams with SVA_MULTI_GATHER_ALL: sva_array_depth_conf
(SVA_FUSE_MEDIAN) against sva_array_depth_sub (SVA_ARRAY_PAIRS, SVA_FUSE_MEDIAN)
as A-B-A blocks of --steps calls each, ms per call.  --array-only-conf runs the
A block alone (the entry an older library has too); SVA_BENCH_ROOT names another
checkout whose built package is timed in place of this one (parent - branch -
parent runs of the existing entry).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("SVA_BENCH_ROOT") or ROOT)


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
            "max": round(max(v), 4)}


def bench_kernels(a, sva, torch, W, H):
    import numpy as np
    ctx = sva.Context(0)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ctx.set_stream(st.cuda_stream)
    np_ = W * H
    out = {}
    for n in a.maps:
        rng = np.random.RandomState(n)
        d = rng.randint(1, 300, size=(n, H, W)).astype(np.uint16)
        d[rng.rand(n, H, W) < 0.2] = 0xFFFF
        s = (d + rng.uniform(-0.5, 0.5, size=d.shape)).astype(np.float32)
        s[d == 0xFFFF] = np.nan
        cmin = rng.randint(40, 48, size=d.shape).astype(np.uint16)
        csec = (cmin + rng.randint(0, 8, size=d.shape)).astype(np.uint16)
        dd, dmin, dsec = (torch.from_numpy(x.view(np.int16)).cuda() for x in (d, cmin, csec))
        ds = torch.from_numpy(s).cuda()
        z = torch.zeros((H, W), dtype=torch.float64, device="cuda")
        nv = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        win = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        b = [0.05 * (1 + i % 5) for i in range(n)]
        f, ps, mm = 0.05, 0.036 / W, sva.SVA_FUSE_MAX_MARGIN
        P = [t.data_ptr() for t in (dd, ds, dmin, dsec, z, nv, win)]
        routes = [
            ("fuse_depth", 2 * n + 9,
             lambda: ctx.fuse_depth_d(P[0], n, W, H, b, f, ps, 0xFFFF, P[4], P[5])),
            ("fuse_depth_sub", 6 * n + 9,
             lambda: ctx.fuse_depth_sub_d(P[0], P[1], n, W, H, b, f, ps, 0xFFFF, P[4], P[5])),
            ("fuse_depth_conf", 6 * n + 10,
             lambda: ctx.fuse_depth_conf_d(P[0], P[2], P[3], n, W, H, b, f, ps, 0xFFFF, mm, P[4],
                                           P[5], P[6])),
            ("fuse_depth_conf_sub", 10 * n + 10,
             lambda: ctx.fuse_depth_conf_sub_d(P[0], P[1], P[2], P[3], n, W, H, b, f, ps, 0xFFFF,
                                               mm, P[4], P[5], P[6])),
        ]
        for _ in range(a.warmup):
            for _, _, run in routes:
                run()
        ctx.synchronize()
        ms = {name: [] for name, _, _ in routes}
        ctx.set_timing(sva.SVA_TIMING_ALL)
        for _ in range(a.steps):
            for name, _, run in routes:
                ctx.reset_timing()
                run()
                ctx.synchronize()
                t, cnt = ctx.kernel_time(name)
                ms[name].append(t / max(cnt, 1))
        ctx.set_timing(sva.SVA_TIMING_OFF)
        row = {}
        for name, bpp, _ in routes:
            sm = summary(ms[name])
            sm["bytes_per_pixel"] = bpp
            sm["GB_per_s"] = round(bpp * np_ / (sm["median"] * 1e-3) / 1e9, 1)
            row[name] = sm
        out["n=%d" % n] = row
    ctx.close()
    return out


def bench_array(a, sva, synth, W, H):
    grid = [(i % 5 - 2, i // 5 - 2) for i in range(25)]
    pairs = [(12, j) for j in (6, 7, 8, 11, 13, 16, 17, 18)]
    kmax = max(synth.pair_step(grid[i], grid[j])[2] for i, j in pairs)
    delta = synth.array_delta(H, W, min((a.D - 1) // kmax, 100))
    views = synth.array_views(H, W, grid, delta, seed=7)
    jobs = []
    for i, j in pairs:
        sx, sy, k = synth.pair_step(grid[i], grid[j])
        jobs.append((i, j, sva.default_params(D=a.D, dir=sx, dir_y=sy), k * 0.05))
    gs, f, ps = [0, len(jobs)], 0.05, 0.036 / W
    m = sva.Multi([0], streams=3, flags=sva.SVA_MULTI_GATHER_RCCL | sva.SVA_MULTI_GATHER_ALL)

    def conf():
        m.array_depth_conf(views, jobs, gs, f, ps, 0, sva.SVA_FUSE_MEDIAN)

    def sub():
        m.array_depth_sub(views, jobs, gs, f, ps, route=sva.SVA_ARRAY_PAIRS,
                          mode=sva.SVA_FUSE_MEDIAN)

    def block(run):
        v = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            run()                                   # the calls are synchronous
            v.append((time.perf_counter() - t0) * 1e3)
        return summary(v)

    try:
        for _ in range(a.warmup):
            conf()
            if not a.array_only_conf:
                sub()
        if a.array_only_conf:
            out = {"array_depth_conf": block(conf)}
        else:
            out = {"A1_array_depth_conf": block(conf), "B_array_depth_sub": block(sub),
                   "A2_array_depth_conf": block(conf)}
    finally:
        m.close()
    return {"pairs": len(jobs), "ms_per_call": out,
            "gathered_bytes_per_pair": {"array_depth_conf": 2 * W * H, "array_depth_sub": 6 * W * H}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--maps", type=int, nargs="+", default=[8, 24])
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--array", action="store_true", help="the center8 frame, A-B-A")
    ap.add_argument("--array-only-conf", action="store_true",
                    help="the center8 frame through sva_array_depth_conf alone")
    a = ap.parse_args()
    import torch
    import stereovisionarray_amd as sva
    from stereovisionarray_amd import synth

    if sva.device_count() < 1:
        raise SystemExit("bench_fuse_sub: no HIP device visible")
    W, H = map(int, a.size.split("x"))
    res = {"size": f"{W}x{H}", "steps": a.steps, "library": sva.LIB_PATH}
    if a.array or a.array_only_conf:
        res["D"] = a.D
        res["array"] = bench_array(a, sva, synth, W, H)
    else:
        res["kernels_ms_per_launch"] = bench_kernels(a, sva, torch, W, H)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
