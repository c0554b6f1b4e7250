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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--uniqueness", type=int, default=10)
    ap.add_argument("--subpixel", type=int, default=1)
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
    ctx.close()
    print(json.dumps({
        "size": f"{W}x{H}", "D": a.D, "steps": a.steps, "subpixel": a.subpixel,
        "uniqueness": a.uniqueness, "reject_share_uniqueness": round(share, 4),
        "reject_share_lr": round(rejected, 4),
        "frame_ms": {n: summary(v) for n, v in frame.items()},
        "wta_hv_ms_per_launch": {n: summary(v) for n, v in wta.items()},
        "sgm_paths_ms_per_launch": {n: summary(v) for n, v in paths.items()},
    }), flush=True)


if __name__ == "__main__":
    main()
