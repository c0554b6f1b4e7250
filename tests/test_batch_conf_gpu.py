"""The batch frame route's confidence form (sva_disparity_sgm_batch_conf_d,
DESIGN.md §2.4b, §4.10): n frames through one sgm_paths and one launch of
wta_hv's confidence instance per sub-batch, the cost planes offset per
sub-batch on the host and per frame in the kernel.

Every frame's disp, cost_min and cost_second must equal the single-frame
confidence route's (sva_disparity_sgm_conf_d) byte for byte, the sub-pixel map
too where it is not NaN; three frames per D are checked against numpy on the
CPU oracle's S volume directly.  Every output is allocated with a guard plane
before and after it (0x5A5A), which a wrong frame offset would touch."""
import functools

import numpy as np
import pytest
import torch

from stereovisionarray_amd import synth

import conf_expect as ce

pytestmark = pytest.mark.gpu

INVALID = 0xFFFF
GUARD16 = 0x5A5A
GUARD32 = 0x5A5A5A5A
SUB_TOL = 1e-5          # the project's sub-pixel tolerance against the oracle (f32 parabola)
STEPS = [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, 1), (-2, -1), (1, -1), (-1, 1)]


def frames(H, W, D, n, seed, steps=STEPS):
    """The frames of test_batch_gpu.py: every frame its own step."""
    out = []
    for i in range(n):
        sx, sy = steps[i % len(steps)]
        if sy == 0:
            L, R, _ = synth.stereo_pair(H, W, D, 0, sx, seed=seed + i, stripes=4, step=5)
        else:
            L, R, _ = synth.stereo_pair2(H, W, D, 0, sx, sy, seed=seed + i, stripes=4, step=5)
        out.append((L, R, sx, sy))
    return out


class Batch:
    """Device inputs of a batch and guarded outputs: [n + 2] planes prefilled
    with the guard value, of which plane 1.. is passed to the library."""

    def __init__(self, sva, dev, fr, D, subpixel=1, invalid=INVALID):
        self.n = len(fr)
        self.H, self.W = fr[0][0].shape
        self.dl = [torch.from_numpy(np.array(L)).to(dev) for L, _, _, _ in fr]
        self.dr = [torch.from_numpy(np.array(R)).to(dev) for _, R, _, _ in fr]
        self.pairs = [(self.dl[i].data_ptr(), self.dr[i].data_ptr(),
                       sva.default_params(D=D, dir=fr[i][2], dir_y=fr[i][3], subpixel=subpixel,
                                          invalid=invalid)) for i in range(self.n)]
        shape = (self.n + 2, self.H, self.W)
        self.maps = torch.full(shape, GUARD16, dtype=torch.int16, device=dev)
        self.cmin = torch.full(shape, GUARD16, dtype=torch.int16, device=dev)
        self.csec = torch.full(shape, GUARD16, dtype=torch.int16, device=dev)
        self.sub = torch.full(shape, GUARD32, dtype=torch.int32, device=dev)

    def run(self, ctx, u, cmin=True, csec=True):
        ctx.disparity_sgm_batch_conf_d(self.pairs, self.W, self.H, self.W, u,
                                       self.maps[1:].data_ptr(), self.sub[1:].data_ptr(),
                                       self.cmin[1:].data_ptr() if cmin else None,
                                       self.csec[1:].data_ptr() if csec else None)

    def fetch(self, ctx):
        """(maps, sub, cmin, csec) of the n frames after checking the guards."""
        ctx.synchronize()
        torch.cuda.synchronize()
        out = []
        for t, guard in ((self.maps, GUARD16), (self.sub, GUARD32), (self.cmin, GUARD16),
                         (self.csec, GUARD16)):
            a = t.cpu().numpy()
            assert (a[0] == guard).all() and (a[-1] == guard).all(), "guard plane written"
            out.append(a[1:-1])
        maps, sub, cmin, csec = out
        return maps.view(np.uint16), sub.view(np.float32), cmin.view(np.uint16), csec.view(np.uint16)


def single(ctx, b, i, u, dev):
    """Frame i through sva_disparity_sgm_conf_d."""
    H, W = b.H, b.W
    d, cm, cs = (torch.zeros((H, W), dtype=torch.int16, device=dev) for _ in range(3))
    s = torch.zeros((H, W), dtype=torch.float32, device=dev)
    ctx.disparity_sgm_conf_d(b.dl[i].data_ptr(), b.dr[i].data_ptr(), W, H, W, b.pairs[i][2], u,
                             d.data_ptr(), s.data_ptr(), cm.data_ptr(), cs.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    return (d.cpu().numpy().view(np.uint16), s.cpu().numpy(), cm.cpu().numpy().view(np.uint16),
            cs.cpu().numpy().view(np.uint16))


def same_sub(got, ref):
    """NaN at the same pixels, equal bits elsewhere."""
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], ref.view(np.uint32)[~nan])


def check_equals_single(ctx, dev, b, u, got):
    maps, sub, cmin, csec = got
    any_rej = False
    for i in range(b.n):
        rd, rs, rmin, rsec = single(ctx, b, i, u, dev)
        assert np.array_equal(maps[i], rd), f"disp frame {i}"
        assert np.array_equal(cmin[i], rmin), f"cost_min frame {i}"
        assert np.array_equal(csec[i], rsec), f"cost_second frame {i}"
        same_sub(sub[i], rs)
        any_rej = any_rej or bool((rd == INVALID).any())
        assert not (rd == INVALID).all()
    assert any_rej == (u > 0), "the reference route's filter must reject some pixels iff u > 0"


@pytest.mark.parametrize("u", [0, 25])
@pytest.mark.parametrize("H,W", [(40, 77), (17, 130)])
@pytest.mark.parametrize("D", [64, 128, 192, 256])
def test_equals_single_frame_conf_route(ctx, sva, torch_dev, D, H, W, u):
    """5 frames: one past a sub-batch of 4."""
    b = Batch(sva, torch_dev, frames(H, W, D, 5, seed=H * W + D), D)
    b.run(ctx, u)
    check_equals_single(ctx, torch_dev, b, u, b.fetch(ctx))


def test_split_route_frames_share_a_census_slot(ctx, sva, torch_dev):
    """test_batch_gpu.py's 7-frame mix of split-route and fused steps."""
    steps = [(1, 3), (-1, 0), (4, 1), (-1, 2), (1, 3), (0, 1), (4, 1)]
    b = Batch(sva, torch_dev, frames(40, 77, 64, 7, seed=40 * 77 + 64, steps=steps), 64)
    b.run(ctx, 25)
    check_equals_single(ctx, torch_dev, b, 25, b.fetch(ctx))


@functools.lru_cache(maxsize=None)
def expect(D, seed, u=10):
    """conf_expect.frame(D, seed) and what the oracle's S volume gives for it."""
    import pyoracle as oracle
    L, R = ce.frame(D, seed)
    S = oracle.aggregate(oracle.cost(oracle.census(L), oracle.census(R), D, 0, -1), threads=8)
    ds, cmin, csec = ce.conf_planes(S)
    rej = ce.rejected(cmin, csec, u)
    disp, sub = oracle.wta(S, 0)
    assert np.array_equal(disp, ds.astype(np.uint16))
    disp, sub = ce.apply_filter(disp, sub, rej, INVALID)
    for a in (L, R, cmin, csec, rej, disp, sub):
        a.setflags(write=False)
    return dict(L=L, R=R, cmin=cmin, csec=csec, rej=rej, disp=disp, sub=sub)


@pytest.mark.parametrize("D", [64, 100, 3])
def test_against_oracle(ctx, sva, torch_dev, D):
    """Three different frames in one batch against numpy on the oracle's S:
    D = 3 has pixels with no second cost, D = 100 runs padded to 128."""
    u = 10
    es = [expect(D, seed) for seed in (7, 8, 9)]
    for e in es:
        if D >= 64:
            assert e["rej"].any() and not e["rej"].all()
        if D == 3:
            assert (e["csec"] == ce.NONE).any()
    b = Batch(sva, torch_dev, [(e["L"], e["R"], -1, 0) for e in es], D)
    b.run(ctx, u)
    maps, sub, cmin, csec = b.fetch(ctx)
    for i, e in enumerate(es):
        assert np.array_equal(cmin[i], e["cmin"]), i
        assert np.array_equal(csec[i], e["csec"]), i
        assert np.array_equal(maps[i], e["disp"]), i
        bad = e["disp"] == INVALID
        assert np.array_equal(np.isnan(sub[i]), bad), i
        assert np.max(np.abs(sub[i][~bad] - e["sub"][~bad]), initial=0.0) <= SUB_TOL, i


def test_past_one_chunk_and_padded_D(ctx, sva, torch_dev):
    """11 frames (two launch sets, 8 + 3), D = 100 (run at 128, padded)."""
    b = Batch(sva, torch_dev, frames(33, 90, 100, 11, seed=5), 100)
    b.run(ctx, 25)
    check_equals_single(ctx, torch_dev, b, 25, b.fetch(ctx))


@pytest.mark.parametrize("which", ["cost_min", "cost_second"])
def test_one_plane_null(ctx, sva, torch_dev, which):
    b = Batch(sva, torch_dev, frames(40, 77, 64, 5, seed=11), 64)
    b.run(ctx, 25, cmin=which != "cost_min", csec=which != "cost_second")
    ctx.synchronize()
    torch.cuda.synchronize()
    off = b.cmin if which == "cost_min" else b.csec
    assert (off.cpu().numpy() == GUARD16).all(), "a NULL plane's neighbour buffer was written"
    maps, sub, cmin, csec = b.fetch(ctx)
    for i in range(b.n):
        rd, rs, rmin, rsec = single(ctx, b, i, 25, torch_dev)
        assert np.array_equal(maps[i], rd), i
        same_sub(sub[i], rs)
        if which == "cost_min":
            assert np.array_equal(csec[i], rsec), i
        else:
            assert np.array_equal(cmin[i], rmin), i


def test_without_subpixel_leaves_subpix_untouched(ctx, sva, torch_dev):
    b = Batch(sva, torch_dev, frames(20, 50, 64, 5, seed=2), 64, subpixel=0)
    b.run(ctx, 25)
    ctx.synchronize()
    torch.cuda.synchronize()
    assert (b.sub.cpu().numpy() == GUARD32).all()
    maps, _, cmin, csec = b.fetch(ctx)
    for i in range(b.n):
        rd, _, rmin, rsec = single(ctx, b, i, 25, torch_dev)
        assert np.array_equal(maps[i], rd) and np.array_equal(cmin[i], rmin)
        assert np.array_equal(csec[i], rsec)


@pytest.mark.parametrize("route", ["conf", "plain"])
def test_subpixel_params_without_a_subpix_buffer(ctx, sva, torch_dev, route):
    """params.subpixel set and subpix NULL, past one sub-batch: no sub-pixel
    map is written anywhere (a NULL base must not be offset per sub-batch)."""
    b = Batch(sva, torch_dev, frames(40, 77, 64, 5, seed=17), 64)
    if route == "conf":
        ctx.disparity_sgm_batch_conf_d(b.pairs, b.W, b.H, b.W, 25, b.maps[1:].data_ptr(), None,
                                       b.cmin[1:].data_ptr(), b.csec[1:].data_ptr())
    else:
        ctx.disparity_sgm_batch_d(b.pairs, b.W, b.H, b.W, b.maps[1:].data_ptr(), None)
    ctx.synchronize()
    torch.cuda.synchronize()
    assert (b.sub.cpu().numpy() == GUARD32).all()
    u = 25 if route == "conf" else 0
    maps = b.maps.cpu().numpy()[1:-1].view(np.uint16)
    for i in range(b.n):
        assert np.array_equal(maps[i], single(ctx, b, i, u, torch_dev)[0]), i


@pytest.mark.parametrize("D", [64, 100])
def test_uniqueness_off_equals_plain_batch(ctx, sva, torch_dev, D):
    b = Batch(sva, torch_dev, frames(40, 77, D, 5, seed=21), D)
    b.run(ctx, 0)
    maps, sub, _, _ = b.fetch(ctx)
    pm = torch.zeros((b.n, b.H, b.W), dtype=torch.int16, device=torch_dev)
    ps = torch.zeros((b.n, b.H, b.W), dtype=torch.float32, device=torch_dev)
    ctx.disparity_sgm_batch_d(b.pairs, b.W, b.H, b.W, pm.data_ptr(), ps.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    assert maps.tobytes() == pm.cpu().numpy().tobytes()
    assert sub.tobytes() == ps.cpu().numpy().tobytes()


def test_back_to_back_calls(ctx, sva, torch_dev):
    """Two calls queued with no synchronisation between them, 9 frames each
    (sub-batches of 4 + 4 + 1 over the side streams)."""
    H, W, D = 36, 70, 64
    calls = [Batch(sva, torch_dev, frames(H, W, D, 9, seed=s), D) for s in (31, 71)]
    for b in calls:
        b.run(ctx, 25)
    for b in calls:
        check_equals_single(ctx, torch_dev, b, 25, b.fetch(ctx))


def test_refusals(ctx, sva, torch_dev):
    H, W = 16, 40
    a = torch.zeros((H, W), dtype=torch.uint8, device=torch_dev)
    out = torch.zeros((2, H, W), dtype=torch.int16, device=torch_dev)
    p0 = sva.default_params(D=64)

    def call(jobs, u):
        with pytest.raises(sva.SvaError) as e:
            ctx.disparity_sgm_batch_conf_d([(a.data_ptr(), a.data_ptr(), p) for p in jobs], W, H, W,
                                           u, out.data_ptr(), None, out.data_ptr(), out.data_ptr())
        return e.value.status

    assert call([p0, p0], -1) == sva.SVA_ERR_INVALID_ARG
    assert call([p0, p0], 101) == sva.SVA_ERR_INVALID_ARG
    assert call([p0, sva.default_params(D=64, invalid=0xFFFE)], 10) == sva.SVA_ERR_INVALID_ARG
    assert call([p0, sva.default_params(D=128)], 10) == sva.SVA_ERR_INVALID_ARG
    assert call([], 10) == sva.SVA_ERR_INVALID_ARG
    assert call([p0, sva.default_params(D=64, lr_check=1)], 10) == sva.SVA_ERR_UNSUPPORTED
    # the plain batch route keeps its refusal of the L/R check
    with pytest.raises(sva.SvaError) as e:
        ctx.disparity_sgm_batch_d([(a.data_ptr(), a.data_ptr(), sva.default_params(D=64, lr_check=1))],
                                  W, H, W, out.data_ptr())
    assert e.value.status == sva.SVA_ERR_UNSUPPORTED


@pytest.mark.parametrize("route", ["conf", "plain"])
def test_fail_cost_switch_is_cleared_by_a_refused_call(ctx, sva, torch_dev, route):
    """SVA_DEBUG_FAIL_COST_AT is for the next batch call: a call that fails
    validation consumes it, and the valid call after it succeeds."""
    D = 64
    b = Batch(sva, torch_dev, frames(20, 50, D, 3, seed=4), D)
    bad = list(b.pairs)
    bad[1] = (bad[1][0], bad[1][1], sva.default_params(D=128))
    ctx.set_debug(sva.SVA_DEBUG_FAIL_COST_AT, 2)
    try:
        with pytest.raises(sva.SvaError) as e:
            if route == "conf":
                ctx.disparity_sgm_batch_conf_d(bad, b.W, b.H, b.W, 25, b.maps[1:].data_ptr())
            else:
                ctx.disparity_sgm_batch_d(bad, b.W, b.H, b.W, b.maps[1:].data_ptr())
        assert e.value.status == sva.SVA_ERR_INVALID_ARG
        assert ctx.get_debug(sva.SVA_DEBUG_FAIL_COST_AT) == 0
    finally:
        ctx.set_debug(sva.SVA_DEBUG_FAIL_COST_AT, 0)
    b.run(ctx, 25)                       # raises if the switch were still armed
    check_equals_single(ctx, torch_dev, b, 25, b.fetch(ctx))
