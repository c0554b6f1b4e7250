#!/usr/bin/env python3
"""The multi-baseline array route against per-pair fusion.

Workload: camera 12 of a 5x5 rig against its eight neighbours (center8), views
from synth.array_views, host images in, depth out, one device, three streams.
  per_pair   sva_array_depth: eight Mode S pipelines, median of the eight maps
  mb         sva_array_depth_mb: eight cost volumes, cost_fuse, ONE aggregation
The two routes alternate A-B-A (per_pair, mb, per_pair) in one session, `--steps`
calls per phase after a warm-up of both; a call is synchronous, so the host clock
around it ends in a device synchronise.  Medians per phase, and the ratio of the
per_pair median (both A phases together) over the mb median.  A last pass with
the per-kernel event timers on gives the mb route's kernel times per call.
--resident leaves the host out: the views live on the device, one context runs
N x sva_disparity_sgm_d + sva_fuse_depth_d against sva_disparity_sgm_multi_d +
sva_fuse_depth_d (one map), each call ending in a synchronise.
Prints one JSON line.

The time of cost_fuse itself comes from a second run under the profiler, with
no counters in it:
  rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- \\
      python tools/bench_multibaseline.py --route mb --steps 10
  python tools/bench_multibaseline.py --stats OUT/.../run_kernel_stats.csv
--stats reads that file and reports the kernel's rate over the model bytes
(N + 1) * W * H * D against the 6.3 TB/s a streaming kernel reaches on this chip.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_TBS = 6.3      # achievable HBM streaming rate (copy kernels), TB/s
KERNELS = ("cost", "cost_fuse", "sgm_paths", "wta_hv", "fuse_depth")


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
            "max": round(max(v), 4), "n": len(v)}


def stats_report(a, W, H):
    rows = list(csv.DictReader(open(a.stats)))
    hit = [r for r in rows if "cost_fuse_kernel" in r["Name"]]
    if not hit:
        raise SystemExit("bench_multibaseline: no cost_fuse_kernel in " + a.stats)
    calls = sum(int(r["Calls"]) for r in hit)
    avg_ns = sum(float(r["TotalDurationNs"]) for r in hit) / calls
    model = (a.pairs + 1) * W * H * a.D
    rate = model / avg_ns / 1e3          # bytes per ns = GB/s; / 1e3 = TB/s
    other = {}
    for r in rows:
        for key in ("sgm_paths_kernel", "wta_hv", "census_cost"):
            if key in r["Name"]:
                other[key] = other.get(key, 0.0) + float(r["TotalDurationNs"]) / 1e6
    print(json.dumps({
        "size": f"{W}x{H}", "D": a.D, "pairs": a.pairs, "cost_fuse_calls": calls,
        "cost_fuse_ms": round(avg_ns / 1e6, 4), "model_bytes": model,
        "cost_fuse_TBps": round(rate, 3), "streaming_TBps": STREAM_TBS,
        "share_of_streaming": round(rate / STREAM_TBS, 3),
        "total_ms_by_kernel": {k: round(v, 3) for k, v in other.items()},
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--pairs", type=int, default=8, help="neighbours of camera 12 used (1..8)")
    ap.add_argument("--steps", type=int, default=20, help="calls per phase")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--route", choices=["both", "mb", "per_pair"], default="both")
    ap.add_argument("--resident", action="store_true",
                    help="device-resident views on one context (sva_disparity_sgm_d x N + "
                         "sva_fuse_depth_d against sva_disparity_sgm_multi_d + depth): no "
                         "staging, no gather")
    ap.add_argument("--stats", help="a rocprofv3 kernel-stats CSV: report cost_fuse's rate")
    a = ap.parse_args()
    W, H = map(int, a.size.split("x"))
    if a.stats:
        return stats_report(a, W, H)

    import stereovisionarray_amd as sva
    from stereovisionarray_amd import synth

    if sva.device_count() < 1:
        raise SystemExit("bench_multibaseline: no HIP device visible")
    grid = [(i % 5 - 2, i // 5 - 2) for i in range(25)]
    pairs = [(12, j) for j in (6, 7, 8, 11, 13, 16, 17, 18)][:a.pairs]
    delta = synth.array_delta(H, W, min(a.D - 1, 100))
    views = synth.array_views(H, W, grid, delta, seed=7)
    jobs = []
    for i, j in pairs:
        sx, sy, k = synth.pair_step(grid[i], grid[j])
        jobs.append((i, j, sva.default_params(D=a.D, dir=sx, dir_y=sy), k * 0.05))
    gs, f, ps = [0, len(jobs)], 0.05, 0.036 / W
    if a.resident:
        # one context, the views on the device, maps and depth left there: no
        # staging, no gather; the per-pair route runs its pairs one after another
        import torch
        ctx = sva.Context(0)
        stream = torch.cuda.Stream()
        torch.cuda.set_stream(stream)
        ctx.set_stream(stream.cuda_stream)
        dv = {v: torch.from_numpy(views[v]).cuda() for v in {12} | {j for _, j in pairs}}
        npair = len(jobs)
        maps = torch.zeros((npair, H, W), dtype=torch.int16, device="cuda")
        depth = torch.zeros((H, W), dtype=torch.float64, device="cuda")
        nvalid = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        bases = [b for *_, b in jobs]
        steps = [(q.dir, q.dir_y) for _, _, q, _ in jobs]
        p0 = sva.default_params(D=a.D)
        cs, close = [ctx], ctx.close

        def per_pair():
            for i, (_, j, q, _) in enumerate(jobs):
                ctx.disparity_sgm_d(dv[12].data_ptr(), dv[j].data_ptr(), W, H, W, q,
                                    maps[i].data_ptr())
            ctx.fuse_depth_d(maps.data_ptr(), npair, W, H, bases, f, ps, 0xFFFF, depth.data_ptr(),
                             nvalid.data_ptr())
            ctx.synchronize()

        def mb():
            ctx.disparity_sgm_multi_d(dv[12].data_ptr(), [dv[j].data_ptr() for _, j in pairs],
                                      steps, W, H, W, p0, 0, maps[0].data_ptr())
            ctx.fuse_depth_d(maps.data_ptr(), 1, W, H, bases[:1], f, ps, 0xFFFF,
                             depth.data_ptr(), nvalid.data_ptr())
            ctx.synchronize()
    else:
        m = sva.Multi([0], streams=a.streams)
        cs, close = [m.context(0, s) for s in range(a.streams)], m.close

        def per_pair():
            return m.array_depth(views, jobs, gs, f, ps)

        def mb():
            return m.array_depth_mb(views, jobs, gs, f, ps)

    routes = {"per_pair": per_pair, "mb": mb}
    phases = {"both": ["per_pair", "mb", "per_pair"], "mb": ["mb"], "per_pair": ["per_pair"]}[a.route]
    try:
        last = {}
        for _ in range(a.warmup):
            for name in sorted(set(phases)):
                last[name] = routes[name]()
        timed = []
        for name in phases:
            v = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                routes[name]()
                v.append((time.perf_counter() - t0) * 1e3)
            timed.append((name, v))
        kernel_ms = {}
        if "mb" in phases:
            for c in cs:
                c.set_timing(sva.SVA_TIMING_ALL)
                c.reset_timing()
            reps = 5
            for _ in range(reps):
                routes["mb"]()
            for k in KERNELS:
                ms = sum(c.kernel_time(k)[0] for c in cs)
                cnt = sum(c.kernel_time(k)[1] for c in cs)
                kernel_ms[k] = {"ms_per_call": round(ms / reps, 4), "launches_per_call": cnt / reps}
            for c in cs:
                c.set_timing(sva.SVA_TIMING_OFF)
    finally:
        close()
    out = {"size": f"{W}x{H}", "D": a.D, "pairs": len(jobs),
           "mode": "resident, one context" if a.resident else "engine, host images",
           "streams": 1 if a.resident else a.streams,
           "steps_per_phase": a.steps,
           "phases": [{"route": n, "ms_per_call": summary(v)} for n, v in timed]}
    by = {}
    for n, v in timed:
        by.setdefault(n, []).extend(v)
    out["ms_per_call"] = {n: summary(v) for n, v in by.items()}
    if len(by) == 2:
        out["per_pair_over_mb"] = round(statistics.median(by["per_pair"]) /
                                        statistics.median(by["mb"]), 3)
    if len(by) == 2 and not a.resident:
        # the share of pixels on which the two routes' depths agree (not a pass bar)
        dp, dm = last["per_pair"][0][0], last["mb"][0][0]
        out["depth_equal_share"] = round(float((dp == dm).mean()), 4)
        out["valid_share"] = {"per_pair": round(float((dp > 0).mean()), 4),
                              "mb": round(float((dm > 0).mean()), 4)}
    if kernel_ms:
        out["mb_kernel_event_ms"] = kernel_ms
        out["cost_fuse_model_bytes"] = (len(jobs) + 1) * W * H * a.D
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
