"""Sub-pixel depth fusion against tests/sub_expect.py, bit for
bit: sva_fuse_depth_sub and sva_fuse_depth_conf_sub take a map's depth from its
f32 sub-pixel disparity, count a map only where that is > 0 (never a NaN), and
with integer-valued sub-pixel maps return the bits of the u16 fusions."""
import ctypes

import numpy as np
import pytest
import torch

import conf_expect as ce
import sub_expect as se
from test_fuse_conf_gpu import maps, W, H, INVALID, F, PS

pytestmark = pytest.mark.gpu

NS = [1, 3, 4, 5, 8, 9, 17, 32]       # one on each side of every unrolled class
BY_D, NONE_AT = (11, 13), (3, 5)      # (row, column): valid by d only / no valid d


def sub_maps(n, seed):
    """maps() of test_fuse_conf_gpu.py with s = d + U(-0.5, 0.5): NaN wherever d
    is invalid or 0, and on valid d about 3 % NaN and a few 0.0f and -1.0f.  At
    BY_D every d is valid and every s NaN; at NONE_AT no d is valid."""
    d, cmin, csec, b = maps(n, seed)
    rng = np.random.RandomState(9000 + seed)
    d[:, BY_D[0], BY_D[1]] = 7
    s = (d.astype(np.float64) + rng.uniform(-0.5, 0.5, size=d.shape)).astype(np.float32)
    by_d = (d != INVALID) & (d != 0)
    s[~by_d] = np.nan
    s[by_d & (rng.rand(*d.shape) < 0.03)] = np.nan
    s[by_d & (rng.rand(*d.shape) < 0.01)] = 0.0
    s[by_d & (rng.rand(*d.shape) < 0.01)] = -1.0
    s[:, BY_D[0], BY_D[1]] = np.nan
    return d, s, cmin, csec, b


def check_coverage(d, s):
    by_d = (d != INVALID) & (d != 0)
    ok = se.valid(d, s, INVALID)
    assert not by_d[:, NONE_AT[0], NONE_AT[1]].any()
    assert by_d[:, BY_D[0], BY_D[1]].all() and not ok[:, BY_D[0], BY_D[1]].any()
    assert (by_d & np.isnan(s)).any() and (by_d & (s == 0)).any() and (by_d & (s < 0)).any()
    assert (ok.sum(0) < by_d.sum(0)).any()
    assert (ok & (s != d)).any()


def same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def on_device(dev, d, s, cmin, csec):
    return (torch.from_numpy(d.view(np.int16)).to(dev), torch.from_numpy(s).to(dev),
            torch.from_numpy(cmin.view(np.int16)).to(dev),
            torch.from_numpy(csec.view(np.int16)).to(dev))


@pytest.mark.parametrize("n", NS)
def test_median(ctx, sva, torch_dev, n):
    d, s, cmin, csec, b = sub_maps(n, 100 + n)
    check_coverage(d, s)
    ez, env, _ = se.fuse_expect(d, s, None, None, b, F, PS, INVALID, se.FUSE_MEDIAN)
    assert env[BY_D] == 0 and env[NONE_AT] == 0 and ez[BY_D] == 0 and not np.isnan(ez).any()
    if n > 1:
        assert ((env > 0) & (env % 2 == 0)).any() and (env % 2 == 1).any()
    z, nv = ctx.fuse_depth_sub(d, s, b, F, PS, INVALID)
    assert same_bits(z, ez) and np.array_equal(nv, env)
    z, nv = ctx.fuse_depth_sub(d, s, b, F, PS, INVALID, want_n_valid=False)
    assert same_bits(z, ez) and nv is None
    # device planes, with and without n_valid
    dd, ds, _, _ = on_device(torch_dev, d, s, cmin, csec)
    for want in (True, False):
        dz = torch.full((H, W), -1.0, dtype=torch.float64, device=torch_dev)
        dn = torch.full((H, W), 77, dtype=torch.uint8, device=torch_dev)
        ctx.fuse_depth_sub_d(dd.data_ptr(), ds.data_ptr(), n, W, H, b, F, PS, INVALID,
                             dz.data_ptr(), dn.data_ptr() if want else None)
        ctx.synchronize()
        torch.cuda.synchronize()
        assert same_bits(dz.cpu().numpy(), ez)
        assert np.array_equal(dn.cpu().numpy(), env if want else np.full((H, W), 77, np.uint8))


@pytest.mark.parametrize("mode", [se.FUSE_MIN_COST, se.FUSE_MAX_MARGIN])
@pytest.mark.parametrize("n", NS)
def test_cost_aware(ctx, sva, torch_dev, n, mode):
    d, s, cmin, csec, b = sub_maps(n, 100 + n)
    ez, env, ew = se.fuse_expect(d, s, cmin, csec, b, F, PS, INVALID, mode)
    assert ew[BY_D] == 0xFF and env[BY_D] == 0 and ew[NONE_AT] == 0xFF
    assert (ew == 0xFF).sum() == (env == 0).sum()
    if n > 1:
        # the sub-pixel rule changes the winner somewhere: the u16 rule's winner is not valid
        _, _, uw = ce.fuse_expect(d, cmin, csec, b, F, PS, INVALID, mode)
        assert ((uw != ew) & (ew != 0xFF)).any()
        assert len(np.unique(ew[env > 0])) > 1
    z, nv, w = ctx.fuse_depth_conf_sub(d, s, cmin, csec, b, F, PS, INVALID, mode)
    assert same_bits(z, ez) and np.array_equal(nv, env) and np.array_equal(w, ew)
    z, nv, w = ctx.fuse_depth_conf_sub(d, s, cmin, csec, b, F, PS, INVALID, mode,
                                       want_n_valid=False, want_winner=False)
    assert same_bits(z, ez) and nv is None and w is None
    dd, ds, dmin, dsec = on_device(torch_dev, d, s, cmin, csec)
    dz = torch.full((H, W), -1.0, dtype=torch.float64, device=torch_dev)
    dn = torch.full((H, W), 77, dtype=torch.uint8, device=torch_dev)
    dw = torch.full((H, W), 77, dtype=torch.uint8, device=torch_dev)
    ctx.fuse_depth_conf_sub_d(dd.data_ptr(), ds.data_ptr(), dmin.data_ptr(), dsec.data_ptr(), n, W,
                              H, b, F, PS, INVALID, mode, dz.data_ptr(), dn.data_ptr(),
                              dw.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    assert same_bits(dz.cpu().numpy(), ez)
    assert np.array_equal(dn.cpu().numpy(), env) and np.array_equal(dw.cpu().numpy(), ew)
    dz.fill_(-1.0)
    ctx.fuse_depth_conf_sub_d(dd.data_ptr(), ds.data_ptr(), dmin.data_ptr(), dsec.data_ptr(), n, W,
                              H, b, F, PS, INVALID, mode, dz.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    assert same_bits(dz.cpu().numpy(), ez)


def test_min_cost_without_cost_second(ctx, sva, torch_dev):
    d, s, cmin, csec, b = sub_maps(5, 7)
    ez, env, ew = se.fuse_expect(d, s, cmin, csec, b, F, PS, INVALID, se.FUSE_MIN_COST)
    z, nv, w = ctx.fuse_depth_conf_sub(d, s, cmin, None, b, F, PS, INVALID, sva.SVA_FUSE_MIN_COST)
    assert same_bits(z, ez) and np.array_equal(nv, env) and np.array_equal(w, ew)
    dd, ds, dmin, _ = on_device(torch_dev, d, s, cmin, csec)
    dz = torch.zeros((H, W), dtype=torch.float64, device=torch_dev)
    ctx.fuse_depth_conf_sub_d(dd.data_ptr(), ds.data_ptr(), dmin.data_ptr(), None, 5, W, H, b, F,
                              PS, INVALID, sva.SVA_FUSE_MIN_COST, dz.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    assert same_bits(dz.cpu().numpy(), ez)


@pytest.mark.parametrize("n", NS)
def test_integer_maps_equal_the_u16_fusions(ctx, sva, n):
    """Identity: s = (float)d, NaN where d is invalid: all three fusions return
    the bits of sva_fuse_depth / sva_fuse_depth_conf."""
    d, cmin, csec, b = maps(n, 100 + n)
    s = d.astype(np.float32)
    s[d == INVALID] = np.nan
    assert (d == 0).any() and np.isnan(s).any()
    z, nv = ctx.fuse_depth_sub(d, s, b, F, PS, INVALID)
    uz, unv = ctx.fuse_depth(d, b, F, PS, INVALID)
    assert same_bits(z, uz) and np.array_equal(nv, unv)
    assert (unv == 0).any() and (uz > 0).any()
    for mode in (sva.SVA_FUSE_MIN_COST, sva.SVA_FUSE_MAX_MARGIN):
        z, nv, w = ctx.fuse_depth_conf_sub(d, s, cmin, csec, b, F, PS, INVALID, mode)
        uz, unv, uw = ctx.fuse_depth_conf(d, cmin, csec, b, F, PS, INVALID, mode)
        assert same_bits(z, uz) and np.array_equal(nv, unv) and np.array_equal(w, uw), mode


def test_kernels_run_under_their_own_timer_names(ctx, sva):
    d, s, cmin, csec, b = sub_maps(5, 3)
    names = ("fuse_depth", "fuse_depth_conf", "fuse_depth_sub", "fuse_depth_conf_sub")
    ctx.reset_timing()
    ctx.set_timing(sva.SVA_TIMING_ALL)
    try:
        ctx.fuse_depth_sub(d, s, b, F, PS, INVALID)
        ctx.fuse_depth_conf_sub(d, s, cmin, csec, b, F, PS, INVALID, sva.SVA_FUSE_MIN_COST)
        ctx.fuse_depth_conf_sub(d, s, cmin, csec, b, F, PS, INVALID, sva.SVA_FUSE_MAX_MARGIN)
        got = {k: ctx.kernel_time(k)[1] for k in names}
    finally:
        ctx.set_timing(sva.SVA_TIMING_OFF)
        ctx.reset_timing()
    assert got == {"fuse_depth": 0, "fuse_depth_conf": 0, "fuse_depth_sub": 1,
                   "fuse_depth_conf_sub": 2}


def test_argument_errors(ctx, sva):
    d, s, cmin, csec, b = sub_maps(3, 1)
    INV = sva.SVA_ERR_INVALID_ARG
    cases = [
        lambda: ctx.fuse_depth_sub(d, None, b, F, PS, INVALID),                    # NULL subpix
        lambda: ctx.fuse_depth_conf_sub(d, None, cmin, csec, b, F, PS, INVALID, 0),
        lambda: ctx.fuse_depth_conf_sub(d, s, cmin, None, b, F, PS, INVALID,
                                        sva.SVA_FUSE_MAX_MARGIN),
        lambda: ctx.fuse_depth_conf_sub(d, s, cmin, csec, b, F, PS, INVALID, 2),   # a bad mode
        lambda: ctx.fuse_depth_conf_sub(d, s, cmin, csec, b, F, PS, INVALID, -1),
    ]
    ctx.reset_timing()
    ctx.set_timing(sva.SVA_TIMING_ALL)
    try:
        for i, call in enumerate(cases):
            with pytest.raises(sva.SvaError) as e:
                call()
            assert e.value.status == INV, i
        # n_maps = 33: the status of the u16 call of each form
        big = np.zeros((33, H, W), np.uint16)
        bigs = np.zeros((33, H, W), np.float32)
        bb = (ctypes.c_double * 33)(*([0.1] * 33))
        out = np.zeros((H, W), np.float64)
        st = sva.lib.sva_fuse_depth_sub(ctx.h, big.ctypes.data, bigs.ctypes.data, 33, W, H, bb, F,
                                        PS, INVALID, out.ctypes.data, None)
        assert st == sva.SVA_ERR_UNSUPPORTED == sva.lib.sva_fuse_depth(
            ctx.h, big.ctypes.data, 33, W, H, bb, F, PS, INVALID, out.ctypes.data, None)
        st = sva.lib.sva_fuse_depth_conf_sub(ctx.h, big.ctypes.data, bigs.ctypes.data,
                                             big.ctypes.data, big.ctypes.data, 33, W, H, bb, F, PS,
                                             INVALID, sva.SVA_FUSE_MIN_COST, out.ctypes.data, None,
                                             None)
        assert st == INV
        dz = torch.zeros((H, W), dtype=torch.float64, device="cuda:0")
        for n in (0, 33):
            with pytest.raises(sva.SvaError):
                ctx.fuse_depth_sub_d(dz.data_ptr(), dz.data_ptr(), n, W, H, [0.1] * max(n, 1), F,
                                     PS, INVALID, dz.data_ptr())
        with pytest.raises(sva.SvaError) as e:
            ctx.fuse_depth_sub_d(dz.data_ptr(), None, 3, W, H, b, F, PS, INVALID, dz.data_ptr())
        assert e.value.status == INV
        with pytest.raises(sva.SvaError) as e:
            ctx.fuse_depth_conf_sub_d(dz.data_ptr(), None, dz.data_ptr(), None, 3, W, H, b, F, PS,
                                      INVALID, 0, dz.data_ptr())
        assert e.value.status == INV
        launched = sum(ctx.kernel_time(k)[1] for k in ("fuse_depth_sub", "fuse_depth_conf_sub"))
    finally:
        ctx.set_timing(sva.SVA_TIMING_OFF)
        ctx.reset_timing()
    assert launched == 0
