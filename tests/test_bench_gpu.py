"""bench.py's N>1 exchange on one GPU: a 1-rank RCCL process group runs the
real overlapped gather (sdist.gather_maps on the comm stream, two map buffers)
and bench.py asserts that the last gathered buffer is the last computed one.
Also checks the driver's JSON contract fields on that line.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_rehearse_rccl_gather():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29573")
    r = subprocess.run([sys.executable, "bench.py", "--steps", "4", "--warmup", "2",
                        "--full", "--no-cpu-baseline", "--rehearse-rccl"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["value"] > 0
    assert "overlapped" in d["config"]["parallelism"]
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and 0 < rf["frac"] < 1
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert rf["traffic"] is None or rf["traffic"] > 0
    fr = d["frame_roofline"]
    assert 0 < fr["frac"] < rf["frac"] and abs(fr["ms_per_frame"] - d["ms_per_step"]) < 1e-3
    # the exchange check (owner checksums, a recomputed unit, timing)
    ex = d["exchange"]
    assert ex["backend"] == "rccl" and ex["rccl_world"] == 1 and ex["ok"]
    assert ex["checksums_ok"] and ex["remote_unit_recomputed"]["equal"]
    assert ex["gather_ms"] > 0 and ex["map_bytes_per_unit"] == 1920 * 1080 * 2


def test_bench_array_rehearse_rccl():
    """The camera-array workload's overlapped gather + fusion on the comm
    stream, through a 1-rank RCCL group (bench.py run_array)."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29575")
    r = subprocess.run([sys.executable, "bench.py", "--workload", "center8", "--steps", "2",
                        "--warmup", "1", "--full", "--no-cpu-baseline", "--rehearse-rccl"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert "overlapped" in d["config"]["parallelism"] and d["config"]["pairs"] == 8
    assert d["exchange"]["ok"] and d["exchange"]["units_checked"] == 8
    # the fused reference depth is the synthetic plane depth on the interior
    assert d["ref_interior_depth_exact_frac"] > 0.98


def test_bench_plain_run_dumps_its_outputs(tmp_path, sva, ctx):
    """A plain run (no --full) times its steps, prints the contract line and,
    with --dump-outputs, writes the last timed step's maps: they must be the
    maps the API returns for the same seeded pair, as float32 .npy files."""
    import numpy as np
    from stereovisionarray_amd import synth
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--workload", "vga_d64",
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["unit"] == "Mdisp/s" and d["higher_is_better"] is True and d["dtype"] == "u16"
    assert abs(d["value"] - 640 * 480 * 64 / (d["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * d["value"]
    # nothing that takes a run of its own
    assert d["cpu_baseline"] is None and "mode_r" not in d and "exchange" not in d
    assert set(d["kernels_ms"]) <= {"sgm_paths", "wta_hv"}
    assert sorted(p.name for p in tmp_path.iterdir()) == ["disparity.npy", "subpixel.npy"]
    L, R, _ = synth.stereo_pair(480, 640, 64, 0, -1, seed=1)
    disp, sub = ctx.disparity_sgm(L, R, sva.default_params(D=64, dmin=0, dir=-1, subpixel=1))
    got_d, got_s = np.load(tmp_path / "disparity.npy"), np.load(tmp_path / "subpixel.npy")
    assert got_d.dtype == np.float32 and got_s.dtype == np.float32
    assert got_d.shape == (1, 480, 640) and got_s.shape == (1, 480, 640)
    assert np.array_equal(got_d[0], disp.astype(np.float32))
    assert np.array_equal(got_s[0].view(np.uint32), sub.view(np.uint32))
