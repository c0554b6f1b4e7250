"""Confidence through the multi-GPU engine and the array route on one MI355X
(sva_batch_sgm_conf_d, sva_array_depth_conf).

As in test_multi_gpu.py the engine runs one device with two streams and the
gather is exercised by routing device 0's own planes through the exchange
(SVA_MULTI_GATHER_ALL, RCCL self send/recv or device-local peer copies).
Every gathered plane equals the single-context confidence route's; the array
frame's maps, cost planes, winners and fused depth (as bits) equal numpy on the
CPU oracle's S volumes (conf_expect)."""
import ctypes as ct
import functools

import numpy as np
import pytest
import torch

from stereovisionarray_amd import synth

import conf_expect as ce

pytestmark = pytest.mark.gpu

MODES = ["rccl_all", "peer_all", "rccl", "peer"]
INVALID = 0xFFFF
GUARD16 = 0x5A5A
GUARD32 = 0x5A5A5A5A


def flags_of(sva, mode):
    f = sva.SVA_MULTI_GATHER_PEER if mode.startswith("peer") else sva.SVA_MULTI_GATHER_RCCL
    return f | (sva.SVA_MULTI_GATHER_ALL if mode.endswith("_all") else 0)


# ---- sva_batch_sgm_conf_d ---------------------------------------------------------
BATCH_STEPS = [(-1, 0), (0, -1), (-1, -1), (1, 0), (-2, -1), (1, 1)]


def batch_jobs(sva):
    """6 pairs, 77 x 40, D = 64, mixed steps; job 1 runs the L/R check, job 2
    marks with 0xFFFE, jobs 3 and 5 have no sub-pixel map."""
    W, H, D = 77, 40, 64
    imgs, ps = [], []
    for i, (sx, sy) in enumerate(BATCH_STEPS):
        if sy == 0:
            L, R, _ = synth.stereo_pair(H, W, D, 0, sx, seed=200 + i, stripes=4, step=5)
        else:
            L, R, _ = synth.stereo_pair2(H, W, D, 0, sx, sy, seed=200 + i, stripes=4, step=5)
        imgs.append((L, R))
        ps.append(sva.default_params(D=D, dir=sx, dir_y=sy, subpixel=0 if i in (3, 5) else 1,
                                     lr_check=1 if i == 1 else 0,
                                     invalid=0xFFFE if i == 2 else INVALID))
    return W, H, imgs, ps


def run_batch_conf(sva, ctx, devices, mode, u, want_min=True, want_sec=True):
    W, H, imgs, ps = batch_jobs(sva)
    n = len(imgs)
    owner = [torch.device("cuda", devices[j % len(devices)]) for j in range(n)]
    d0 = torch.device("cuda", devices[0])
    m = sva.Multi(devices, streams=2, flags=flags_of(sva, mode))
    try:
        dl = [torch.from_numpy(a).to(owner[j]) for j, (a, _) in enumerate(imgs)]
        dr = [torch.from_numpy(b).to(owner[j]) for j, (_, b) in enumerate(imgs)]
        shape = (n + 2, H, W)
        maps = torch.full(shape, GUARD16, dtype=torch.int16, device=d0)
        cmin = torch.full(shape, GUARD16, dtype=torch.int16, device=d0)
        csec = torch.full(shape, GUARD16, dtype=torch.int16, device=d0)
        sub = torch.full(shape, GUARD32, dtype=torch.int32, device=d0)
        for d in devices:
            torch.cuda.synchronize(d)
        jobs = [(dl[j].data_ptr(), dr[j].data_ptr(), ps[j]) for j in range(n)]
        for _ in range(2):                      # the second call reuses the slots
            m.batch_sgm_conf_d(jobs, W, H, W, u, maps[1:].data_ptr(), sub[1:].data_ptr(),
                               cmin[1:].data_ptr() if want_min else None,
                               csec[1:].data_ptr() if want_sec else None)
            m.synchronize()
        got = [t.cpu().numpy() for t in (maps, sub, cmin, csec)]
    finally:
        m.close()
    for a, guard in zip(got, (GUARD16, GUARD32, GUARD16, GUARD16)):
        assert (a[0] == guard).all() and (a[-1] == guard).all(), "guard plane written"
    gm, gs, gmin, gsec = (a[1:-1] for a in got)
    if not want_min:
        assert (gmin == GUARD16).all()
    if not want_sec:
        assert (gsec == GUARD16).all()
    any_rej = False
    for j, (L, R) in enumerate(imgs):
        ed, es, emin, esec = ctx.disparity_sgm_conf(L, R, ps[j], u)
        any_rej = any_rej or bool((ed == ps[j].invalid).any())
        assert not (ed == ps[j].invalid).all()
        assert np.array_equal(gm[j].view(np.uint16), ed), f"disp {j}"
        if want_min:
            assert np.array_equal(gmin[j].view(np.uint16), emin), f"cost_min {j}"
        if want_sec:
            assert np.array_equal(gsec[j].view(np.uint16), esec), f"cost_second {j}"
        if ps[j].subpixel:
            nan = np.isnan(es)
            got_s = gs[j].view(np.float32)
            assert np.array_equal(np.isnan(got_s), nan), f"sub {j}"
            assert np.array_equal(got_s.view(np.uint32)[~nan], es.view(np.uint32)[~nan]), f"sub {j}"
        else:
            assert (gs[j] == GUARD32).all(), f"sub plane of job {j} written"
    assert any_rej
    assert (gm[2].view(np.uint16) == 0xFFFE).any() and not (gm[2].view(np.uint16) == INVALID).any()


@pytest.mark.parametrize("mode", MODES)
def test_batch_sgm_conf_d(ctx, sva, mode):
    run_batch_conf(sva, ctx, [0], mode, 25)


@pytest.mark.parametrize("which", ["cost_min", "cost_second"])
@pytest.mark.parametrize("mode", ["rccl_all", "peer_all"])
def test_batch_sgm_conf_d_one_plane_null(ctx, sva, mode, which):
    run_batch_conf(sva, ctx, [0], mode, 25, want_min=which != "cost_min",
                   want_sec=which != "cost_second")


def test_batch_sgm_conf_d_refuses_bad_uniqueness(sva, torch_dev):
    m = sva.Multi([0], streams=1, flags=sva.SVA_MULTI_GATHER_PEER)
    try:
        a = torch.zeros((16, 40), dtype=torch.uint8, device=torch_dev)
        out = torch.zeros((1, 16, 40), dtype=torch.int16, device=torch_dev)
        for u in (-1, 101):
            with pytest.raises(sva.SvaError) as e:
                m.batch_sgm_conf_d([(a.data_ptr(), a.data_ptr(), sva.default_params(D=64))], 40, 16,
                                   40, u, out.data_ptr())
            assert e.value.status == sva.SVA_ERR_INVALID_ARG
    finally:
        m.close()


# ---- sva_array_depth_conf ---------------------------------------------------------
W, H, D = 160, 128, 64
PITCH_M, F, PS = 0.05, 0.05, 0.036 / 160


def _mini_rig():
    """The rig of test_multi_gpu.py: camera 4 of a 3x3 grid against its 8
    neighbours, plus camera 0 against 1 and 3: two fusion groups."""
    grid = [(i % 3 - 1, i // 3 - 1) for i in range(9)]
    pairs = [(4, j) for j in (0, 1, 2, 3, 5, 6, 7, 8)] + [(0, 1), (0, 3)]
    return grid, pairs, [0, 8, 10]


@functools.lru_cache(maxsize=None)
def rig(seed=3):
    """Views, jobs and every pair's (d*, cost_min, cost_second) from the CPU
    oracle's S volume, computed once."""
    import pyoracle as oracle
    import stereovisionarray_amd as sva
    grid, pairs, gs = _mini_rig()
    views = synth.array_views(H, W, grid, synth.array_delta(H, W, 14), seed=seed)
    cen = [oracle.census(v) for v in views]
    jobs, ds, cmin, csec = [], [], [], []
    for i, j in pairs:
        sx, sy, k = synth.pair_step(grid[i], grid[j])
        jobs.append((i, j, sva.default_params(D=D, dir=sx, dir_y=sy), k * PITCH_M))
        S = oracle.aggregate(oracle.cost2(cen[i], cen[j], D, 0, sx, sy), threads=8)
        a, b, c = ce.conf_planes(S)
        ds.append(a.astype(np.uint16))
        cmin.append(b)
        csec.append(c)
    ds, cmin, csec = np.stack(ds), np.stack(cmin), np.stack(csec)
    for a in (ds, cmin, csec):
        a.setflags(write=False)
    return dict(views=views, jobs=jobs, gs=gs, ds=ds, cmin=cmin, csec=csec,
                bases=[b for *_, b in jobs])


@functools.lru_cache(maxsize=None)
def filtered(u, seed=3):
    """The expected maps at uniqueness u."""
    r = rig(seed)
    rej = ce.rejected(r["cmin"], r["csec"], u)
    maps = np.where(rej, np.uint16(INVALID), r["ds"]).astype(np.uint16)
    maps.setflags(write=False)
    return maps, rej


@functools.lru_cache(maxsize=None)
def fused(u, mode, seed=3):
    """[(depth, n_valid, winner)] per group, conf_expect.fuse_expect."""
    r = rig(seed)
    maps, _ = filtered(u, seed)
    out = []
    for g in range(len(r["gs"]) - 1):
        sl = slice(r["gs"][g], r["gs"][g + 1])
        out.append(ce.fuse_expect(maps[sl], r["cmin"][sl], r["csec"][sl], r["bases"][sl], F, PS,
                                  INVALID, mode))
    return out


def check_preconditions():
    """What the rig must contain, asserted on the expected planes."""
    for j in range(10):
        share = float(filtered(25)[1][j].mean())
        assert 0.02 <= share <= 0.6, (j, share)
    for u in (0, 25):
        wins = {}
        for mode in (ce.FUSE_MIN_COST, ce.FUSE_MAX_MARGIN):
            _, nv, win = fused(u, mode)[0]
            wins[mode] = win
            for k in range(8):
                assert int((win == k).sum()) >= 100, (u, mode, k)
            assert (nv == 0).any(), u
        both = (wins[0] != 0xFF)
        assert float((wins[0][both] != wins[1][both]).mean()) >= 0.30, u


def check_conf_result(res, u, mode, want=True):
    r = rig()
    depth, nv, win, maps, cmin, csec = res
    emaps, _ = filtered(u)
    if want:
        assert np.array_equal(maps, emaps), f"maps: {int((maps != emaps).sum())} differ"
        assert np.array_equal(cmin, r["cmin"])
        assert np.array_equal(csec, r["csec"])
    else:
        assert maps is None and cmin is None and csec is None
    for g, (ez, en, ew) in enumerate(fused(u, mode)):
        assert np.array_equal(nv[g], en), g
        assert np.array_equal(win[g], ew), g
        assert np.array_equal(depth[g].view(np.uint64), ez.view(np.uint64)), g


@pytest.mark.parametrize("fuse", ["min_cost", "max_margin"])
@pytest.mark.parametrize("mode", MODES)
def test_array_depth_conf_matches_oracle(sva, mode, fuse):
    check_preconditions()
    fm = sva.SVA_FUSE_MIN_COST if fuse == "min_cost" else sva.SVA_FUSE_MAX_MARGIN
    r = rig()
    m = sva.Multi([0], streams=2, flags=flags_of(sva, mode))
    try:
        res = {u: m.array_depth_conf(r["views"], r["jobs"], r["gs"], F, PS, u, fm, want_maps=True,
                                     want_costs=True) for u in (0, 25)}
        # the planes the mode needs are gathered also when the caller asks for none
        bare = m.array_depth_conf(r["views"], r["jobs"], r["gs"], F, PS, 25, fm)
    finally:
        m.close()
    for u in (0, 25):
        check_conf_result(res[u], u, fm)
    check_conf_result(bare, 25, fm, want=False)


@pytest.mark.parametrize("mode", ["rccl_all", "peer"])
def test_array_depth_conf_median(sva, oracle, mode):
    r = rig()
    m = sva.Multi([0], streams=2, flags=flags_of(sva, mode))
    try:
        d25, n25, w25, m25, min25, sec25 = m.array_depth_conf(
            r["views"], r["jobs"], r["gs"], F, PS, 25, sva.SVA_FUSE_MEDIAN, want_maps=True,
            want_costs=True)
        d0, n0, w0, m0, _, _ = m.array_depth_conf(r["views"], r["jobs"], r["gs"], F, PS, 0,
                                                  sva.SVA_FUSE_MEDIAN, want_maps=True)
        pd, pn, pm = m.array_depth(r["views"], r["jobs"], r["gs"], F, PS, want_maps=True)
    finally:
        m.close()
    assert w25 is None and w0 is None
    emaps, rej = filtered(25)
    assert rej.any()
    assert np.array_equal(m25, emaps)
    assert np.array_equal(min25, r["cmin"]) and np.array_equal(sec25, r["csec"])
    for g in range(len(r["gs"]) - 1):
        sl = slice(r["gs"][g], r["gs"][g + 1])
        ez, en = oracle.fuse_depth(np.array(emaps[sl]), r["bases"][sl], F, PS)
        assert np.array_equal(n25[g], en)
        assert np.array_equal(d25[g].view(np.uint64), ez.view(np.uint64))
    assert d0.tobytes() == pd.tobytes() and n0.tobytes() == pn.tobytes()
    assert m0.tobytes() == pm.tobytes()


def test_array_depth_conf_engine_reuse(sva):
    """conf, plain, conf on one engine: the slot layout changes between calls."""
    r = rig()
    m = sva.Multi([0], streams=2, flags=flags_of(sva, "rccl_all"))
    try:
        a = m.array_depth_conf(r["views"], r["jobs"], r["gs"], F, PS, 25, sva.SVA_FUSE_MAX_MARGIN,
                               want_maps=True, want_costs=True)
        pd, pn, pm = m.array_depth(r["views"], r["jobs"], r["gs"], F, PS, want_maps=True)
        b = m.array_depth_conf(r["views"], r["jobs"], r["gs"], F, PS, 25, sva.SVA_FUSE_MAX_MARGIN,
                               want_maps=True, want_costs=True)
    finally:
        m.close()
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    check_conf_result(a, 25, sva.SVA_FUSE_MAX_MARGIN)
    assert np.array_equal(pm, rig()["ds"])


def test_array_depth_conf_refusals(sva):
    m = sva.Multi([0], streams=1, flags=sva.SVA_MULTI_GATHER_PEER)
    try:
        v = [np.zeros((24, 24), np.uint8)] * 3
        p0 = sva.default_params(D=64)
        jobs = [(0, 1, p0, 0.05), (0, 2, p0, 0.05)]
        for u, mode in ((0, 3), (101, sva.SVA_FUSE_MIN_COST), (-1, sva.SVA_FUSE_MEDIAN)):
            with pytest.raises(sva.SvaError) as e:
                m.array_depth_conf(v, jobs, [0, 2], 0.05, 1e-4, u, mode)
            assert e.value.status == sva.SVA_ERR_INVALID_ARG, (u, mode)
        p1 = sva.default_params(D=64)
        p1.invalid = 0
        with pytest.raises(sva.SvaError) as e:
            m.array_depth_conf(v, [(0, 1, p0, 0.05), (0, 2, p1, 0.05)], [0, 2], 0.05, 1e-4, 10,
                               sva.SVA_FUSE_MIN_COST)
        assert e.value.status == sva.SVA_ERR_INVALID_ARG
        # a winner plane with the median (the Python wrapper never passes one)
        ptrs = (ct.c_void_p * 3)(*[a.ctypes.data for a in v])
        jp = (sva.ArrayPair * 2)(sva.ArrayPair(0, 1, p0, 0.05), sva.ArrayPair(0, 2, p0, 0.05))
        gs = (ct.c_int32 * 2)(0, 2)
        depth = np.zeros((24, 24), np.float64)
        win = np.zeros((24, 24), np.uint8)
        st = sva.lib.sva_array_depth_conf(m.h, ptrs, 3, 24, 24, 24, jp, 2, gs, 1, 0.05, 1e-4, 10,
                                          sva.SVA_FUSE_MEDIAN, depth.ctypes.data, None,
                                          win.ctypes.data, None, None, None)
        assert st == sva.SVA_ERR_INVALID_ARG
    finally:
        m.close()


# ---- several devices: skipped on a one-GPU box -----------------------------------
def _devices(sva):
    n = min(sva.device_count(), 4)
    if n < 2:
        pytest.skip("needs >= 2 HIP devices")
    return list(range(n))


@pytest.mark.parametrize("mode", ["rccl", "peer"])
def test_batch_sgm_conf_d_across_devices(ctx, sva, mode):
    run_batch_conf(sva, ctx, _devices(sva), mode, 25)


@pytest.mark.parametrize("mode", ["rccl", "peer"])
def test_array_depth_conf_across_devices(sva, mode):
    devs = _devices(sva)
    r = rig()
    m = sva.Multi(devs, streams=2, flags=flags_of(sva, mode))
    try:
        res = m.array_depth_conf(r["views"], r["jobs"], r["gs"], F, PS, 25,
                                 sva.SVA_FUSE_MAX_MARGIN, want_maps=True, want_costs=True)
    finally:
        m.close()
    check_conf_result(res, 25, sva.SVA_FUSE_MAX_MARGIN)
