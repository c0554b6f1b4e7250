#!/usr/bin/env python3
"""Mixed-baseline Mode S: the cost_mixed kernel against
the equal-baseline cost kernels, and one fused 24-pair frame against today's
two-group use of the same views.

--kernel: per step in (1,0), (1,1), (2,1), the event-timer time of one launch of
  cost_mixed at ratios 2/1 and 1/2 (sva_cost_mixed_d, from census maps),
  cost_split   the cost kernel from the same census maps at ratio 1 (sva_cost_d),
  cost_fused   census + cost in one kernel from the images (sva_census_cost_d),
`--steps` launches each after a warm-up, kinds interleaved round by round; the
mean per launch, cost_mixed's ratio to each, and its bytes per second over the
W*H*D bytes written.

default (frame): camera 12 of the 5x5 rig against all 24 others, views resident
on one context, each call ending in a synchronise, phases A-B-A in one session:
  A  two sva_disparity_sgm_multi_d (the inner 8; the outer ring of 16 at its own
     disparity scale) + sva_fuse_depth_d of the two maps
  B  one sva_disparity_sgm_mixed_d (unit = the long baseline) + sva_fuse_depth_d
Medians per phase, A over B, and a last pass of B with the event timers on: the
per-kernel times per call, and the break-even arithmetic of §4.20 from them.
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("census", "cost", "cost_mixed", "cost_fuse", "sgm_paths", "wta_hv", "fuse_depth")
KERNEL_STEPS = [(1, 0), (1, 1), (2, 1)]


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
            "max": round(max(v), 4), "n": len(v)}


def context(sva):
    import torch
    ctx = sva.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    return ctx


def kernel_level(a, W, H):
    import torch
    import stereovisionarray_amd as sva
    from stereovisionarray_amd import synth

    ctx = context(sva)
    L, R, _ = synth.stereo_pair(H, W, a.D, 0, 1, seed=7)
    dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    cl = torch.zeros((H, W), dtype=torch.int64, device="cuda")
    cr = torch.zeros((H, W), dtype=torch.int64, device="cuda")
    C = torch.zeros((H, W, a.D), dtype=torch.uint8, device="cuda")
    ctx.census_d(dl.data_ptr(), W, H, W, cl.data_ptr())
    ctx.census_d(dr.data_ptr(), W, H, W, cr.data_ptr())
    ctx.synchronize()
    rows = []
    try:
        for sx, sy in KERNEL_STEPS:
            p = sva.default_params(D=a.D, dir=sx, dir_y=sy)
            kinds = {
                "cost_mixed_2_1": ("cost_mixed", lambda: ctx.cost_mixed_d(
                    cl.data_ptr(), cr.data_ptr(), W, H, a.D, a.D, 0, (sx, sy), (2, 1), C.data_ptr())),
                "cost_mixed_1_2": ("cost_mixed", lambda: ctx.cost_mixed_d(
                    cl.data_ptr(), cr.data_ptr(), W, H, a.D, a.D, 0, (sx, sy), (1, 2), C.data_ptr())),
                "cost_split": ("cost", lambda: ctx.cost_d(cl.data_ptr(), cr.data_ptr(), W, H, p,
                                                          C.data_ptr())),
                "cost_fused": ("cost", lambda: ctx.census_cost_d(dl.data_ptr(), dr.data_ptr(), W,
                                                                 H, W, p, C.data_ptr())),
            }
            ms = {k: [] for k in kinds}
            ctx.set_timing(sva.SVA_TIMING_ALL)
            for it in range(a.warmup + a.steps):
                for k, (timer, call) in kinds.items():
                    ctx.reset_timing()
                    call()
                    ctx.synchronize()
                    t, n = ctx.kernel_time(timer)
                    assert n == 1
                    if it >= a.warmup:
                        ms[k].append(t)
            ctx.set_timing(sva.SVA_TIMING_OFF)
            med = {k: statistics.median(v) for k, v in ms.items()}
            row = {"step": [sx, sy], "ms": {k: summary(v) for k, v in ms.items()}}
            for k in ("cost_mixed_2_1", "cost_mixed_1_2"):
                row[k + "_over_split"] = round(med[k] / med["cost_split"], 3)
                row[k + "_over_fused"] = round(med[k] / med["cost_fused"], 3)
                row[k + "_TBps_written"] = round(W * H * a.D / med[k] / 1e9, 3)
            rows.append(row)
    finally:
        ctx.close()
    print(json.dumps({"size": f"{W}x{H}", "D": a.D, "steps": a.steps, "kernel_level": rows}),
          flush=True)


def frame_level(a, W, H):
    import torch
    import stereovisionarray_amd as sva
    from stereovisionarray_amd import synth

    grid = [(i % 5 - 2, i // 5 - 2) for i in range(25)]
    others = [j for j in range(25) if j != 12]
    # per-grid-unit disparity up to (D - 1) / 2: the long baseline's range is D
    delta = synth.array_delta(H, W, max(5, min((a.D - 1) // 2, 50)))
    views = synth.array_views(H, W, grid, delta, seed=7)
    steps, ks = [], []
    for j in others:
        sx, sy, k = synth.pair_step(grid[12], grid[j])
        steps.append((sx, sy))
        ks.append(k)
    inner = [i for i, k in enumerate(ks) if k == 1]
    outer = [i for i, k in enumerate(ks) if k == 2]
    assert len(inner) == 8 and len(outer) == 16
    ratios = [(k, 2) if k == 1 else (1, 1) for k in ks]
    f, ps, pitch = 0.05, 0.036 / W, 0.05
    ctx = context(sva)
    dv = [torch.from_numpy(v).cuda() for v in views]
    ptr = [dv[j].data_ptr() for j in others]
    maps = torch.zeros((2, H, W), dtype=torch.int16, device="cuda")
    depth = torch.zeros((H, W), dtype=torch.float64, device="cuda")
    nvalid = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    p_in = sva.default_params(D=max(1, a.D // 2))      # the short baseline sees half the range
    p0 = sva.default_params(D=a.D)

    def two_groups():
        ctx.disparity_sgm_multi_d(dv[12].data_ptr(), [ptr[i] for i in inner],
                                  [steps[i] for i in inner], W, H, W, p_in, 0, maps[0].data_ptr())
        ctx.disparity_sgm_multi_d(dv[12].data_ptr(), [ptr[i] for i in outer],
                                  [steps[i] for i in outer], W, H, W, p0, 0, maps[1].data_ptr())
        ctx.fuse_depth_d(maps.data_ptr(), 2, W, H, [pitch, 2 * pitch], f, ps, 0xFFFF,
                         depth.data_ptr(), nvalid.data_ptr())
        ctx.synchronize()

    def mixed():
        ctx.disparity_sgm_mixed_d(dv[12].data_ptr(), ptr, steps, ratios, W, H, W, p0, 0,
                                  maps[0].data_ptr())
        ctx.fuse_depth_d(maps.data_ptr(), 1, W, H, [2 * pitch], f, ps, 0xFFFF, depth.data_ptr(),
                         nvalid.data_ptr())
        ctx.synchronize()

    routes = {"two_groups": two_groups, "mixed": mixed}
    phases = {"both": ["two_groups", "mixed", "two_groups"], "mixed": ["mixed"],
              "two_groups": ["two_groups"]}[a.route]
    try:
        for _ in range(a.warmup):
            for name in sorted(set(phases)):
                routes[name]()
        timed = []
        for name in phases:
            v = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                routes[name]()
                v.append((time.perf_counter() - t0) * 1e3)
            timed.append((name, v))
        kernel_ms = {}
        reps = 5
        for name in sorted(set(phases)):
            ctx.set_timing(sva.SVA_TIMING_ALL)
            ctx.reset_timing()
            for _ in range(reps):
                routes[name]()
            kernel_ms[name] = {}
            for k in KERNELS:
                ms, cnt = ctx.kernel_time(k)
                if cnt:
                    kernel_ms[name][k] = {"ms_per_call": round(ms / reps, 4),
                                          "launches_per_call": cnt / reps,
                                          "ms_per_launch": round(ms / cnt, 4)}
            ctx.set_timing(sva.SVA_TIMING_OFF)
    finally:
        ctx.close()
    out = {"size": f"{W}x{H}", "D": a.D, "pairs": 24, "mode": "resident, one context",
           "steps_per_phase": a.steps,
           "phases": [{"route": n, "ms_per_call": summary(v)} for n, v in timed]}
    by = {}
    for n, v in timed:
        by.setdefault(n, []).extend(v)
    out["ms_per_call"] = {n: summary(v) for n, v in by.items()}
    if len(by) == 2:
        out["two_groups_over_mixed"] = round(statistics.median(by["two_groups"]) /
                                             statistics.median(by["mixed"]), 3)
    out["kernel_event_ms"] = kernel_ms
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20, help="calls per phase / launches per kind")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--route", choices=["both", "mixed", "two_groups"], default="both")
    ap.add_argument("--kernel", action="store_true", help="the kernel-level comparison")
    a = ap.parse_args()
    W, H = map(int, a.size.split("x"))
    import stereovisionarray_amd as sva
    if sva.device_count() < 1:
        raise SystemExit("bench_mixed: no HIP device visible")
    (kernel_level if a.kernel else frame_level)(a, W, H)


if __name__ == "__main__":
    main()
