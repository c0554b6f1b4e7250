"""Different aggregation plans carved in turn over one context's two
workspaces (csrc/agg_plan.h).  The per-route suites pin each
route to the oracle on its own; here one context, reserved once, runs a
pair-route frame, a batch of three, a four-volume frame, a confidence frame,
the stage entries on caller buffers and the pair-route frame again, at two
sizes and at a native and a padded D.  Every output must be bit-equal to the
same call on a fresh context, the first frame's to the oracle, and
SVA_DEBUG_DIAG_ROUTE tells after each frame that it took the route meant."""
import numpy as np
import pytest
import torch

from stereovisionarray_amd import synth

pytestmark = pytest.mark.gpu

PAIR, FOUR = 1, 0
CASES = [(90, 37, 128), (90, 37, 100), (65, 31, 128), (65, 31, 100)]
BATCH_STEPS = [(-1, 0), (1, 0), (-1, -1)]


def params(sva, D, **kw):
    return sva.default_params(D=D, dmin=0, dir=-1, P1=10, subpixel=1, **kw)


def pair_frame(c, sva, dev, oracle, L, R, D):
    return c.disparity_sgm(L, R, params(sva, D, P2=120)), PAIR


def four_frame(c, sva, dev, oracle, L, R, D):
    return c.disparity_sgm(L, R, params(sva, D, P2=128)), FOUR


def conf_frame(c, sva, dev, oracle, L, R, D):
    return c.disparity_sgm_conf(L, R, params(sva, D, P2=120), uniqueness=10), PAIR


def batch(c, sva, dev, oracle, L, R, D):
    H, W = L.shape
    imgs = []
    for i, (sx, sy) in enumerate(BATCH_STEPS):
        if sy == 0:
            A, B, _ = synth.stereo_pair(H, W, D, 0, sx, seed=40 + i, stripes=4, step=5)
        else:
            A, B, _ = synth.stereo_pair2(H, W, D, 0, sx, sy, seed=40 + i, stripes=4, step=5)
        imgs.append((torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)))
    pairs = [(a.data_ptr(), b.data_ptr(),
              sva.default_params(D=D, dmin=0, dir=sx, dir_y=sy, subpixel=1))
             for (a, b), (sx, sy) in zip(imgs, BATCH_STEPS)]
    maps = torch.full((3, H, W), 0x5A5A, dtype=torch.int16, device=dev)
    sub = torch.zeros((3, H, W), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    c.disparity_sgm_batch_d(pairs, W, H, W, maps.data_ptr(), sub.data_ptr())
    c.synchronize()
    return (maps.cpu().numpy(), sub.cpu().numpy()), None


def stages(c, sva, dev, oracle, L, R, D):
    """paths_tile_d + wta_hv_d at the native width, on buffers of tile_layout."""
    H, W = L.shape
    Dp = 128
    C = torch.from_numpy(oracle.cost(oracle.census(L), oracle.census(R), Dp, 0, -1)).to(dev)
    lay = sva.tile_layout(W, H, Dp)
    assert C.numel() == lay.cost_bytes
    diag = torch.full((lay.diag_bytes,), 0xAB, dtype=torch.uint8, device=dev)
    hck = torch.full((lay.hckpt_bytes,), 0xCD, dtype=torch.uint8, device=dev)
    vck = torch.full((lay.vckpt_bytes,), 0xEF, dtype=torch.uint8, device=dev)
    disp = torch.zeros((H, W), dtype=torch.int16, device=dev)
    sub = torch.zeros((H, W), dtype=torch.float32, device=dev)
    p = params(sva, Dp, P2=120)
    torch.cuda.synchronize()
    c.paths_tile_d(C.data_ptr(), C.numel(), W, H, p, diag.data_ptr(), diag.numel(),
                   hck.data_ptr(), hck.numel(), vck.data_ptr(), vck.numel())
    c.wta_hv_d(C.data_ptr(), C.numel(), diag.data_ptr(), diag.numel(), hck.data_ptr(),
               hck.numel(), vck.data_ptr(), vck.numel(), W, H, p, disp.data_ptr(), sub.data_ptr())
    c.synchronize()
    return tuple(t.cpu().numpy() for t in (disp, sub, diag, hck, vck)), None


STEPS = [("pair frame", pair_frame), ("batch of 3", batch), ("four-volume frame", four_frame),
         ("confidence frame", conf_frame), ("stage entries", stages),
         ("pair frame again", pair_frame)]


def run_step(c, sva, dev, oracle, fn, L, R, D):
    """(outputs, the route meant, the route reported) of one step on context c.
    Only a frame reports a route; the batch and the stage entries leave the
    last frame's."""
    before = c.get_debug(sva.SVA_DEBUG_DIAG_ROUTE)
    out, want = fn(c, sva, dev, oracle, L, R, D)
    return out, before if want is None else want, c.get_debug(sva.SVA_DEBUG_DIAG_ROUTE)


@pytest.fixture(scope="module")
def runs(sva, oracle, torch_dev):
    """{case: (L, R, [(step, run_step on the shared context, on a fresh one)])}:
    every case in turn on one reserved context, every step also on a context
    of its own."""
    if sva.device_count() < 1:
        pytest.fail("GPU test selected but no HIP device is visible")
    shared = sva.Context(0)
    shared.set_debug(sva.SVA_DEBUG_DIAG_PAIR_MIN_PIXELS, 0)
    shared.reserve(90, 37, 128)
    out = {}
    try:
        for W, H, D in CASES:
            L, R, _ = synth.stereo_pair(H, W, D, 0, -1, seed=W + D)
            rows = []
            for name, fn in STEPS:
                a = run_step(shared, sva, torch_dev, oracle, fn, L, R, D)
                fresh = sva.Context(0)
                try:
                    fresh.set_debug(sva.SVA_DEBUG_DIAG_PAIR_MIN_PIXELS, 0)
                    b = run_step(fresh, sva, torch_dev, oracle, fn, L, R, D)
                finally:
                    fresh.close()
                rows.append((name, a, b))
            out[(W, H, D)] = (L, R, rows)
    finally:
        shared.set_debug(sva.SVA_DEBUG_DIAG_PAIR_MIN_PIXELS, -1)
        shared.close()
    return out


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-D%d" % c)
def test_shared_workspace_equals_fresh_context(runs, case):
    _, _, rows = runs[case]
    assert [r[0] for r in rows] == [s[0] for s in STEPS]
    for name, (out_a, want_a, got_a), (out_b, want_b, got_b) in rows:
        assert got_a == want_a, f"{name}: route on the shared context"
        assert got_b == want_b, f"{name}: route on the fresh context"
        assert len(out_a) == len(out_b)
        for i, (x, y) in enumerate(zip(out_a, out_b)):
            assert same_bits(x, y), f"{name}: output {i}"
    # the pair frame before and after the other plans
    for x, y in zip(rows[0][1][0], rows[-1][1][0]):
        assert same_bits(x, y)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-D%d" % c)
def test_first_frame_equals_oracle(runs, oracle, case):
    W, H, D = case
    L, R, rows = runs[case]
    disp, sub = rows[0][1][0]
    od, osub = oracle.sgm(L, R, D, 0, -1, 10, 120, subpixel=True, threads=4)
    assert np.array_equal(disp, od)
    assert np.max(np.abs(sub - osub)) <= 1e-5
