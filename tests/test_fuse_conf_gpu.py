"""Cost-aware depth fusion (SURVEY.md §8e "or min-cost")
against a numpy f64 expectation, bit for bit: sva_fuse_depth_conf picks, per
pixel, the valid map with the smallest cost_min or the largest
cost_second - cost_min, ties to the lowest map index.
"""
import ctypes

import numpy as np
import pytest
import torch

from stereovisionarray_amd import synth

import conf_expect as ce

pytestmark = pytest.mark.gpu

W, H = 83, 41
INVALID = 0xFFFF
F, PS = 0.05, 0.036 / 640


def maps(n, seed):
    """Random u16 disparities (about a fifth invalid, some 0), costs from 8
    values so that ties across maps are common, one pixel with no valid map."""
    rng = np.random.RandomState(seed)
    d = rng.randint(1, 300, size=(n, H, W)).astype(np.uint16)
    d[rng.rand(n, H, W) < 0.2] = INVALID
    d[rng.rand(n, H, W) < 0.05] = 0
    d[:, 3, 5] = INVALID
    d[: (n + 1) // 2, 7, 9] = 0
    d[(n + 1) // 2:, 7, 9] = INVALID
    cmin = rng.randint(40, 48, size=(n, H, W)).astype(np.uint16)
    csec = (cmin + rng.randint(0, 8, size=(n, H, W))).astype(np.uint16)
    csec[rng.rand(n, H, W) < 0.03] = ce.NONE      # no second cost: the largest margin
    b = 0.05 * (1 + np.arange(n) % 5)
    return d, cmin, csec, b


@pytest.mark.parametrize("mode", [ce.FUSE_MIN_COST, ce.FUSE_MAX_MARGIN])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 8, 9, 17, 32])
def test_fuse_conf(ctx, sva, n, mode):
    """One n on each side of every unrolled map-count class (4, 8, 16, 32)."""
    d, cmin, csec, b = maps(n, 100 + n)
    ez, env, ew = ce.fuse_expect(d, cmin, csec, b, F, PS, INVALID, mode)
    assert (env == 0).any() and (ew == 0xFF).sum() == (env == 0).sum()
    if n > 1:
        score = cmin.astype(np.int64) if mode == ce.FUSE_MIN_COST else \
            (csec.astype(np.uint32) - cmin.astype(np.uint32)).astype(np.int64)
        ok = (d != INVALID) & (d != 0)
        best = np.where(ok, score, -1).max(0) if mode else np.where(ok, score, 1 << 40).min(0)
        assert (((score == best) & ok).sum(0) > 1).any()      # ties between valid maps
        assert len(np.unique(ew[env > 0])) > 1
    z, nv, w = ctx.fuse_depth_conf(d, cmin, csec, b, F, PS, INVALID, mode)
    assert np.array_equal(z.view(np.uint64), ez.view(np.uint64))
    assert np.array_equal(nv, env)
    assert np.array_equal(w, ew)


def test_min_cost_without_cost_second(ctx, sva, torch_dev):
    d, cmin, csec, b = maps(5, 7)
    ez, env, ew = ce.fuse_expect(d, cmin, csec, b, F, PS, INVALID, ce.FUSE_MIN_COST)
    z, nv, w = ctx.fuse_depth_conf(d, cmin, None, b, F, PS, INVALID, sva.SVA_FUSE_MIN_COST)
    assert np.array_equal(z.view(np.uint64), ez.view(np.uint64))
    assert np.array_equal(nv, env) and np.array_equal(w, ew)
    # device buffers, n_valid and winner left out
    dd, dc = (torch.from_numpy(a.view(np.int16)).to(torch_dev) for a in (d, cmin))
    dz = torch.zeros((H, W), dtype=torch.float64, device=torch_dev)
    ctx.fuse_depth_conf_d(dd.data_ptr(), dc.data_ptr(), None, 5, W, H, b, F, PS, INVALID,
                          sva.SVA_FUSE_MIN_COST, dz.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(dz.cpu().numpy().view(np.uint64), ez.view(np.uint64))


def test_argument_errors(ctx, sva):
    d, cmin, csec, b = maps(3, 1)
    with pytest.raises(sva.SvaError) as e:
        ctx.fuse_depth_conf(d, cmin, None, b, F, PS, INVALID, sva.SVA_FUSE_MAX_MARGIN)
    assert e.value.status == sva.SVA_ERR_INVALID_ARG
    with pytest.raises(sva.SvaError) as e:
        ctx.fuse_depth_conf(d, cmin, csec, b, F, PS, INVALID, 2)
    assert e.value.status == sva.SVA_ERR_INVALID_ARG
    big = np.zeros((33, H, W), np.uint16)
    bb = (ctypes.c_double * 33)(*([0.1] * 33))
    out = np.zeros((H, W), np.float64)
    st = sva.lib.sva_fuse_depth_conf(ctx.h, big.ctypes.data, big.ctypes.data, big.ctypes.data, 33,
                                     W, H, bb, F, PS, INVALID, sva.SVA_FUSE_MIN_COST,
                                     out.ctypes.data, None, None)
    assert st == sva.SVA_ERR_INVALID_ARG


def test_array_end_to_end(ctx, sva, oracle):
    """Three pairs of one reference camera of a synthetic array, matched with
    disparity_sgm_conf (uniqueness 10) and fused in both modes."""
    D, Hh, Ww = 64, 72, 120
    grid = synth.array_grid(2, 4)
    delta = synth.array_delta(Hh, Ww, 14, stripes=5)
    views = synth.array_views(Hh, Ww, grid, delta, seed=3)
    disps, cmins, csecs, base = [], [], [], []
    for j in (1, 2, 4):                       # camera 0 against (1,0), (2,0), (0,1)
        sx, sy, k = synth.pair_step(grid[0], grid[j])
        p = sva.default_params(D=D, dir=sx, dir_y=sy, invalid=INVALID)
        disp, _, cmin, csec = ctx.disparity_sgm_conf(views[0], views[j], p, 10)
        S = oracle.aggregate(oracle.cost2(oracle.census(views[0]), oracle.census(views[j]), D, 0,
                                          sx, sy), threads=8)
        ds, ecmin, ecsec = ce.conf_planes(S)
        exp, _ = ce.apply_filter(ds.astype(np.uint16), None, ce.rejected(ecmin, ecsec, 10), INVALID)
        assert np.array_equal(disp, exp) and np.array_equal(cmin, ecmin)
        assert np.array_equal(csec, ecsec)
        disps.append(disp); cmins.append(cmin); csecs.append(csec); base.append(0.05 * k)
    d, cm, cs = np.stack(disps), np.stack(cmins), np.stack(csecs)
    for mode in (sva.SVA_FUSE_MIN_COST, sva.SVA_FUSE_MAX_MARGIN):
        ez, env, ew = ce.fuse_expect(d, cm, cs, base, F, PS, INVALID, mode)
        assert len(np.unique(ew[env > 0])) == 3       # every map wins somewhere
        z, nv, w = ctx.fuse_depth_conf(d, cm, cs, base, F, PS, INVALID, mode)
        assert np.array_equal(z.view(np.uint64), ez.view(np.uint64))
        assert np.array_equal(nv, env) and np.array_equal(w, ew)
