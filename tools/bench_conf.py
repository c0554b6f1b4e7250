#!/usr/bin/env python3
"""What the WTA confidence route costs: sva_disparity_sgm_d
against sva_disparity_sgm_conf_d on one warm context, alternating step by step,
with the L/R check (the other filter) next to them.

Routes, run round-robin so that drift hits all of them alike:
  plain      sva_disparity_sgm_d
  conf       sva_disparity_sgm_conf_d, both cost planes, uniqueness 0
  conf_u     the same with --uniqueness (the filter costs nothing extra)
  lr         sva_disparity_sgm_d with lr_check = 1 (a second full pass)
Frame time: host clock around one call that ends in a stream synchronise, timers
off.  Kernel time: a second round with SVA_TIMING_AGG, the `wta_hv` and
`sgm_paths` totals read back and reset after every step (both wta_hv instances
keep that timer name).  Prints one JSON line; medians, with min and max.

--batch N adds the batch frame route on N frames of the same size (DESIGN.md
§4.10), ms per call, round-robin like the rows above:
  batch_plain   sva_disparity_sgm_batch_d
  batch_conf    sva_disparity_sgm_batch_conf_d, both cost planes, uniqueness 0
  batch_conf_u  the same with --uniqueness
--array adds the array route on the center8 rig (camera 12 of a 5x5 grid against
its eight neighbours) at the same size, host images in, fused depth out, ms per
call, on an engine of one device and three streams with device 0's planes routed
through the gather (SVA_MULTI_GATHER_ALL), and the bytes gathered per pair:
  array_plain       sva_array_depth
  array_median      sva_array_depth_conf, SVA_FUSE_MEDIAN
  array_min_cost    sva_array_depth_conf, SVA_FUSE_MIN_COST
  array_max_margin  sva_array_depth_conf, SVA_FUSE_MAX_MARGIN
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
            "max": round(max(v), 4)}


BATCH_STEPS = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]


def timed_rounds(routes, steps, warmup, sync):
    """ms per call of every route, run round-robin."""
    for _ in range(warmup):
        for _, run in routes:
            run()
    sync()
    out = {n: [] for n, _ in routes}
    for _ in range(steps):
        for n, run in routes:
            t0 = time.perf_counter()
            run()
            sync()
            out[n].append((time.perf_counter() - t0) * 1e3)
    return {n: summary(v) for n, v in out.items()}


def bench_batch(a, sva, synth, torch, ctx, W, H):
    n = a.batch
    fr = []
    for i in range(n):
        sx, sy = BATCH_STEPS[i % len(BATCH_STEPS)]
        L, R, _ = synth.stereo_pair2(H, W, a.D, 0, sx, sy, seed=1 + i)
        fr.append((torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), sx, sy))
    pairs = [(l.data_ptr(), r.data_ptr(),
              sva.default_params(D=a.D, dir=sx, dir_y=sy, subpixel=a.subpixel))
             for l, r, sx, sy in fr]
    maps, cmin, csec = (torch.zeros((n, H, W), dtype=torch.int16, device="cuda") for _ in range(3))
    sub = torch.zeros((n, H, W), dtype=torch.float32, device="cuda")

    def conf(u):
        ctx.disparity_sgm_batch_conf_d(pairs, W, H, W, u, maps.data_ptr(), sub.data_ptr(),
                                       cmin.data_ptr(), csec.data_ptr())

    routes = [("batch_plain", lambda: ctx.disparity_sgm_batch_d(pairs, W, H, W, maps.data_ptr(),
                                                                sub.data_ptr())),
              ("batch_conf", lambda: conf(0)), ("batch_conf_u", lambda: conf(a.uniqueness))]
    return {"frames": n, "ms_per_call": timed_rounds(routes, a.steps, a.warmup, ctx.synchronize)}


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

    def conf(mode):
        return lambda: m.array_depth_conf(views, jobs, gs, f, ps, a.uniqueness, mode)

    routes = [("array_plain", lambda: m.array_depth(views, jobs, gs, f, ps)),
              ("array_median", conf(sva.SVA_FUSE_MEDIAN)),
              ("array_min_cost", conf(sva.SVA_FUSE_MIN_COST)),
              ("array_max_margin", conf(sva.SVA_FUSE_MAX_MARGIN))]
    try:
        ms = timed_rounds(routes, a.steps, a.warmup, lambda: None)     # the calls are synchronous
    finally:
        m.close()
    planes = {"array_plain": 1, "array_median": 1, "array_min_cost": 2, "array_max_margin": 3}
    return {"pairs": len(jobs), "ms_per_call": ms,
            "gathered_bytes_per_pair": {n: 2 * W * H * k for n, k in planes.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--uniqueness", type=int, default=10)
    ap.add_argument("--subpixel", type=int, default=1)
    ap.add_argument("--batch", type=int, default=0, help="frames of the batch rows (0 = none)")
    ap.add_argument("--array", action="store_true", help="add the array-route rows")
    a = ap.parse_args()
    import torch
    import stereovisionarray_amd as sva
    from stereovisionarray_amd import synth

    if sva.device_count() < 1:
        raise SystemExit("bench_conf: no HIP device visible")
    W, H = map(int, a.size.split("x"))
    ctx = sva.Context(0)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ctx.set_stream(st.cuda_stream)
    L, R, _ = synth.stereo_pair(H, W, a.D, 0, -1, seed=1)
    dL, dR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    disp = torch.zeros((H, W), dtype=torch.int16, device="cuda")
    sub = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    cmin = torch.zeros((H, W), dtype=torch.int16, device="cuda")
    csec = torch.zeros((H, W), dtype=torch.int16, device="cuda")
    p = sva.default_params(D=a.D, dir=-1, subpixel=a.subpixel)
    plr = sva.default_params(D=a.D, dir=-1, subpixel=a.subpixel, lr_check=1)
    ptr = [t.data_ptr() for t in (dL, dR, disp, sub, cmin, csec)]

    def plain(q):
        ctx.disparity_sgm_d(ptr[0], ptr[1], W, H, W, q, ptr[2], ptr[3])

    def conf(u):
        ctx.disparity_sgm_conf_d(ptr[0], ptr[1], W, H, W, p, u, ptr[2], ptr[3], ptr[4], ptr[5])

    routes = [("plain", lambda: plain(p)), ("conf", lambda: conf(0)),
              ("conf_u", lambda: conf(a.uniqueness)), ("lr", lambda: plain(plr))]
    ctx.reserve(W, H, a.D)
    for _ in range(a.warmup):
        for _, run in routes:
            run()
    ctx.synchronize()

    frame = {n: [] for n, _ in routes}
    for _ in range(a.steps):
        for n, run in routes:
            t0 = time.perf_counter()
            run()
            ctx.synchronize()
            frame[n].append((time.perf_counter() - t0) * 1e3)

    wta = {n: [] for n, _ in routes}
    paths = {n: [] for n, _ in routes}
    ctx.set_timing(sva.SVA_TIMING_AGG)
    for _ in range(a.steps):
        for n, run in routes:
            ctx.reset_timing()
            run()
            ctx.synchronize()
            ms, cnt = ctx.kernel_time("wta_hv")
            wta[n].append(ms / max(cnt, 1))
            ms, cnt = ctx.kernel_time("sgm_paths")
            paths[n].append(ms / max(cnt, 1))
    ctx.set_timing(sva.SVA_TIMING_OFF)
    plain(plr)
    ctx.synchronize()
    rejected = float((disp.cpu().numpy().view("uint16") == p.invalid).mean())
    conf(a.uniqueness)
    ctx.synchronize()
    share = float((disp.cpu().numpy().view("uint16") == p.invalid).mean())
    extra = {}
    if a.batch > 0:
        extra["batch"] = bench_batch(a, sva, synth, torch, ctx, W, H)
    ctx.close()
    if a.array:
        extra["array"] = bench_array(a, sva, synth, W, H)
    print(json.dumps({
        "size": f"{W}x{H}", "D": a.D, "steps": a.steps, "subpixel": a.subpixel,
        "uniqueness": a.uniqueness, "reject_share_uniqueness": round(share, 4),
        "reject_share_lr": round(rejected, 4),
        "frame_ms": {n: summary(v) for n, v in frame.items()},
        "wta_hv_ms_per_launch": {n: summary(v) for n, v in wta.items()},
        "sgm_paths_ms_per_launch": {n: summary(v) for n, v in paths.items()},
        **extra,
    }), flush=True)


if __name__ == "__main__":
    main()
