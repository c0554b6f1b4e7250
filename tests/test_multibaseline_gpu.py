"""Multi-baseline Mode S on the GPU.

Bars: the fusion stage bit-exact against mb_expect.fuse on random volumes; the
frame route's disparity and cost planes bit-exact against oracle.cost2 ->
mb_expect.fuse -> oracle.aggregate -> oracle.wta / conf_expect.conf_planes,
sub-pixel within the project's 1e-5; the array route's maps equal to the
single-context route and its depth bit-exact against oracle.fuse_depth."""
import ctypes as ct
import functools

import numpy as np
import pytest
import torch

from stereovisionarray_amd import synth

import conf_expect as ce
import mb_expect
from test_array_gpu import SPLIT_STEPS

pytestmark = pytest.mark.gpu

SUB_TOL = 1e-5
NEIGHBOURS = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]
STAGE_STEPS = NEIGHBOURS + [(2, -1), (-1, 3), (-3, -2), (2, 2)]
SW, SH = 37, 23          # the stage frame: narrower than every D
COUNTED = ("census", "cost", "cost_fuse", "sgm_paths", "wta_hv")


def stage_steps(n):
    return [STAGE_STEPS[i % len(STAGE_STEPS)] for i in range(n)]


@functools.lru_cache(maxsize=None)
def stage_volumes(D):
    """32 uniformly random u8 volumes [SH][SW][D], read-only."""
    rng = np.random.default_rng(4000 + D)
    v = rng.integers(0, 256, size=(32, SH, SW, D), dtype=np.uint8)
    v.setflags(write=False)
    return v


def run_stage(ctx, dev, vols, stride, steps, D, dreal, dmin):
    """vols: device u8 buffer holding the volumes `stride` bytes apart."""
    out = torch.zeros((SH, SW, D), dtype=torch.uint8, device=dev)
    ctx.cost_fuse_d(vols.data_ptr(), stride, steps, SW, SH, D, dreal, dmin, out.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 8, 9, 16, 17, 32])
@pytest.mark.parametrize("D", [64, 128, 192, 256])
def test_cost_fuse_stage(ctx, torch_dev, D, N):
    V = stage_volumes(D)[:N]
    steps = stage_steps(N)
    vols = torch.from_numpy(V.copy()).to(torch_dev)
    for dmin in (0, 9):
        cnt = mb_expect.counts(SW, SH, D, dmin, steps)
        assert (cnt == 0).any() and (cnt == N).any()
        if N > 1:
            assert ((cnt > 0) & (cnt < N)).any()
        for dreal in (D, D - 1, D - 37):
            exp = mb_expect.fuse(list(V), steps, dmin, dreal)
            got = run_stage(ctx, torch_dev, vols, SH * SW * D, steps, D, dreal, dmin)
            assert np.array_equal(got, exp), (dmin, dreal, int((got != exp).sum()))


def test_cost_fuse_stage_stride_larger_than_volume(ctx, torch_dev):
    D, N, dmin, dreal = 128, 5, 9, 100
    V = stage_volumes(D)[:N]
    nv = SH * SW * D
    stride = nv + 4096 + 48
    rng = np.random.default_rng(5)
    buf = rng.integers(0, 256, size=stride * N, dtype=np.uint8)    # the gaps hold noise
    for i in range(N):
        buf[i * stride:i * stride + nv] = V[i].ravel()
    steps = stage_steps(N)
    got = run_stage(ctx, torch_dev, torch.from_numpy(buf).to(torch_dev), stride, steps, D, dreal,
                    dmin)
    assert np.array_equal(got, mb_expect.fuse(list(V), steps, dmin, dreal))


def test_cost_fuse_stage_stride_beyond_32_bits(ctx, torch_dev):
    """N = 2 volumes 2^32 + 4096 bytes apart in one allocation.  A volume base
    formed in 32 bits would wrap to byte 4096 of the same buffer, which lies
    inside volume 0 and holds other data: a wrong kernel fails the comparison,
    it cannot fault."""
    free, _ = torch.cuda.mem_get_info(torch_dev)
    if free < 10 * (1 << 30):
        pytest.skip("needs 10 GB of free device memory")
    D, dmin = 64, 0
    V = stage_volumes(D)[:2]
    nv = SH * SW * D
    assert nv > 4096 + 4096
    stride = (1 << 32) + 4096
    buf = torch.empty(stride + nv, dtype=torch.uint8, device=torch_dev)
    buf[:nv] = torch.from_numpy(V[0].ravel().copy()).to(torch_dev)
    buf[stride:stride + nv] = torch.from_numpy(V[1].ravel().copy()).to(torch_dev)
    assert not np.array_equal(V[0].ravel()[4096:8192], V[1].ravel()[:4096])
    steps = stage_steps(2)
    got = run_stage(ctx, torch_dev, buf, stride, steps, D, D, dmin)
    del buf
    assert np.array_equal(got, mb_expect.fuse(list(V), steps, dmin, D))


# ---- frame route ---------------------------------------------------------------
def _grid3():
    return [(i % 3 - 1, i // 3 - 1) for i in range(9)]


# name -> (W, H, D, dmin, grid, reference camera, matched cameras)
FRAMES = {
    "n8_d64": (96, 80, 64, 0, _grid3(), 4, [0, 1, 2, 3, 5, 6, 7, 8]),
    "n4_dmin3": (96, 80, 64, 3, _grid3(), 4, [1, 3, 5, 7]),
    "n3_d40_padded": (131, 75, 40, 2, _grid3(), 0, [1, 3, 4]),
    "n8_d128": (150, 110, 128, 0, _grid3(), 4, [0, 1, 2, 3, 5, 6, 7, 8]),
    # the outer ring of a 5x5 rig around its centre: every baseline has major component 2
    "ring_2_1": (96, 80, 64, 0, [(0, 0), (2, 1), (-2, 1), (1, -2), (2, 0), (-2, -2)], 0,
                 [1, 2, 3, 4, 5]),
    # major component 3; (1, 3) is a step no census+cost kernel takes
    "split_step": (96, 80, 64, 0, [(0, 0), (-1, -3), (-3, -1), (0, 3)], 0, [1, 2, 3]),
}


@functools.lru_cache(maxsize=None)
def frame(name):
    """Views, steps and the expected planes of one frame, computed once."""
    import pyoracle as oracle
    W, H, D, dmin, grid, r, others = FRAMES[name]
    steps, ks = [], set()
    for j in others:
        sx, sy, k = synth.pair_step(grid[r], grid[j])
        steps.append((sx, sy))
        ks.add(k)
    assert len(ks) == 1                  # one disparity is one depth in every pair
    k = ks.pop()
    delta = synth.array_delta(H, W, max(5, min((D - 1) // k - dmin, 14)))
    views = synth.array_views(H, W, grid, delta, seed=11)
    cen = [oracle.census(v) for v in views]
    Cs = [oracle.cost2(cen[r], cen[j], D, dmin, sx, sy) for j, (sx, sy) in zip(others, steps)]
    Cf = mb_expect.fuse(Cs, steps, dmin)
    S = oracle.aggregate(Cf, threads=8)
    disp, sub = oracle.wta(S, dmin, subpixel=True)
    ds, cmin, csec = ce.conf_planes(S)
    assert np.array_equal(disp, (ds + dmin).astype(np.uint16))
    for a in (Cf, disp, sub, cmin, csec):
        a.setflags(write=False)
    return dict(W=W, H=H, D=D, dmin=dmin, ref=views[r], others=[views[j] for j in others],
                steps=steps, Cs=Cs, Cf=Cf, disp=disp, sub=sub, cmin=cmin, csec=csec)


def test_frames_cover_the_step_classes():
    assert any(abs(sx) == 2 and abs(sy) == 1 for sx, sy in frame("ring_2_1")["steps"])
    assert any(s in SPLIT_STEPS for s in frame("split_step")["steps"])
    for name in FRAMES:
        f = frame(name)
        cnt = mb_expect.counts(f["W"], f["H"], f["D"], f["dmin"], f["steps"])
        assert ((cnt > 0) & (cnt < len(f["steps"]))).any(), name


@pytest.mark.parametrize("u", [0, 10])
@pytest.mark.parametrize("name", list(FRAMES))
def test_frame_route(ctx, sva, name, u):
    f = frame(name)
    p = sva.default_params(D=f["D"], dmin=f["dmin"], dir=0, dir_y=0, subpixel=1)
    disp, sub, cmin, csec = ctx.disparity_sgm_multi(f["ref"], f["others"], f["steps"], p, u)
    assert np.array_equal(cmin, f["cmin"])
    assert np.array_equal(csec, f["csec"])
    rej = ce.rejected(f["cmin"], f["csec"], u)
    edisp, esub = ce.apply_filter(f["disp"], f["sub"], rej)
    assert np.array_equal(disp, edisp)
    assert np.array_equal(np.isnan(sub), rej)
    assert np.max(np.abs(sub[~rej] - esub[~rej])) <= SUB_TOL
    if u:
        assert rej.any() and (~rej).any()
        assert (disp == p.invalid).any() and (disp != p.invalid).any()
    else:
        assert not rej.any()


def test_frame_route_plain_instance(ctx, sva):
    """No plane and no uniqueness: the plain WTA instance, the same map."""
    f = frame("n4_dmin3")
    p = sva.default_params(D=f["D"], dmin=f["dmin"], subpixel=0)
    W, H = f["W"], f["H"]
    dev = torch.device("cuda:0")
    imgs = [torch.from_numpy(a).to(dev) for a in [f["ref"]] + f["others"]]
    disp = torch.zeros((H, W), dtype=torch.int16, device=dev)
    ctx.disparity_sgm_multi_d(imgs[0].data_ptr(), [t.data_ptr() for t in imgs[1:]], f["steps"], W,
                              H, W, p, 0, disp.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(disp.cpu().numpy().view(np.uint16), f["disp"])


def test_one_pair_equals_the_pair_route(ctx, sva):
    f = frame("n8_d64")
    for j in (0, 3, 6):
        sx, sy = f["steps"][j]
        p = sva.default_params(D=f["D"], dmin=f["dmin"], dir=sx, dir_y=sy, subpixel=1)
        one = ctx.disparity_sgm_multi(f["ref"], [f["others"][j]], [(sx, sy)], p, 10)
        pair = ctx.disparity_sgm_conf(f["ref"], f["others"][j], p, 10)
        for a, b in zip(one, pair):
            assert a.tobytes() == b.tobytes()


def test_pair_order_does_not_matter(ctx, sva):
    f = frame("n8_d64")
    p = sva.default_params(D=f["D"], dmin=f["dmin"], subpixel=1)
    base = ctx.disparity_sgm_multi(f["ref"], f["others"], f["steps"], p, 10)
    order = [5, 2, 7, 0, 3, 6, 1, 4]
    shuf = ctx.disparity_sgm_multi(f["ref"], [f["others"][i] for i in order],
                                   [f["steps"][i] for i in order], p, 10)
    for a, b in zip(base, shuf):
        assert a.tobytes() == b.tobytes()


def counts_of(ctx):
    return {k: ctx.kernel_time(k)[1] for k in COUNTED}


def test_kernel_counts(ctx, sva):
    f = frame("n8_d64")
    p = sva.default_params(D=f["D"], dmin=f["dmin"])
    ctx.reset_timing()
    ctx.set_timing(sva.SVA_TIMING_ALL)
    try:
        ctx.disparity_sgm_multi(f["ref"], f["others"], f["steps"], p, 0)
        got = counts_of(ctx)
    finally:
        ctx.set_timing(sva.SVA_TIMING_OFF)
        ctx.reset_timing()
    assert got == {"census": 0, "cost": 8, "cost_fuse": 1, "sgm_paths": 1, "wta_hv": 1}


def test_refusals_launch_nothing(ctx, sva, torch_dev):
    f = frame("n4_dmin3")
    W, H, D = f["W"], f["H"], f["D"]
    ref, oth, steps = f["ref"], f["others"], f["steps"]
    good = sva.default_params(D=D, dmin=f["dmin"])
    lr = sva.default_params(D=D, dmin=f["dmin"], lr_check=1)
    bigd = sva.default_params(D=300)
    badp = sva.default_params(D=D, P2=200)
    INV, UNS = sva.SVA_ERR_INVALID_ARG, sva.SVA_ERR_UNSUPPORTED

    def multi(others, st, p, u=0):
        return lambda: ctx.disparity_sgm_multi(ref, others, st, p, u)

    def raw(others_ptrs, n):
        """The C entry point with a hand-made image list (a null image)."""
        def call():
            disp = np.zeros((H, W), np.uint16)
            ptrs = (ct.c_void_p * n)(*others_ptrs)
            st = (ct.c_int32 * (2 * n))(*[v for s in steps[:n] for v in s])
            ctx._chk(sva.lib.sva_disparity_sgm_multi(ctx.h, ref.ctypes.data, ptrs, st, n, W, H, W,
                                                     ct.byref(good), 0, disp.ctypes.data, None,
                                                     None, None))
        return call

    vol = torch.zeros((2, H, W, 64), dtype=torch.uint8, device=torch_dev)
    out = torch.zeros((H, W, 64), dtype=torch.uint8, device=torch_dev)
    nv = H * W * 64

    def stage(n=2, D=64, dreal=64, dmin=0, st=((1, 0), (0, 1)), stride=nv, v=vol, o=out):
        return lambda: ctx.cost_fuse_d(v.data_ptr() if v is not None else None, stride,
                                       list(st)[:n] if n <= len(st) else list(st) * 17, W, H, D,
                                       dreal, dmin, o.data_ptr() if o is not None else None)

    cases = [
        (multi([], [], good), INV),                                    # n = 0
        (multi(oth * 9, steps * 9, good), INV),                         # n = 36
        (raw([oth[0].ctypes.data, None], 2), INV),                      # a null image
        (multi(oth, [steps[0], (0, 0)] + steps[2:], good), INV),        # a zero step
        (multi(oth, steps, lr), UNS),
        (multi(oth, steps, bigd), UNS),                                 # check_sgm
        (multi(oth, steps, badp), INV),                                 # check_sgm
        (multi(oth, steps, good, 101), INV),                            # check_uniqueness
        (stage(n=34), INV),
        (stage(st=((1, 0), (0, 0))), INV),
        (stage(D=100, dreal=100), UNS),
        (stage(dreal=0), INV),
        (stage(dreal=65), INV),
        (stage(stride=nv - 16), INV),
        (stage(stride=nv + 8), INV),
        (stage(v=None), INV),
        (stage(o=None), INV),
    ]
    ctx.reset_timing()
    ctx.set_timing(sva.SVA_TIMING_ALL)
    try:
        for i, (call, status) in enumerate(cases):
            with pytest.raises(sva.SvaError) as e:
                call()
            assert e.value.status == status, i
        got = counts_of(ctx)
    finally:
        ctx.set_timing(sva.SVA_TIMING_OFF)
        ctx.reset_timing()
    assert got == dict.fromkeys(COUNTED, 0)


# ---- array route ---------------------------------------------------------------
AW, AH, AD = 96, 80, 64
PITCH_M, F, PS = 0.05, 0.05, 0.036 / 160
FLAGS = {"rccl_all": lambda s: s.SVA_MULTI_GATHER_RCCL | s.SVA_MULTI_GATHER_ALL,
         "peer": lambda s: s.SVA_MULTI_GATHER_PEER, "rccl": lambda s: s.SVA_MULTI_GATHER_RCCL}


@functools.lru_cache(maxsize=None)
def rig():
    """A 3x3 grid, two groups: camera 4 with its 8 neighbours, camera 0 with its 3."""
    import stereovisionarray_amd as sva
    grid = _grid3()
    pairs = [(4, j) for j in (0, 1, 2, 3, 5, 6, 7, 8)] + [(0, 1), (0, 3), (0, 4)]
    views = synth.array_views(AH, AW, grid, synth.array_delta(AH, AW, 14), seed=3)
    jobs = []
    for i, j in pairs:
        sx, sy, k = synth.pair_step(grid[i], grid[j])
        jobs.append((i, j, sva.default_params(D=AD, dir=sx, dir_y=sy), k * PITCH_M))
    return dict(views=views, jobs=jobs, gs=[0, 8, 11])


def check_array(sva, ctx, oracle, res, u):
    r = rig()
    depth, maps, cmin, csec = res
    for g in range(2):
        js = r["jobs"][r["gs"][g]:r["gs"][g + 1]]
        p = sva.default_params(D=AD)
        one = ctx.disparity_sgm_multi(r["views"][js[0][0]], [r["views"][j] for _, j, _, _ in js],
                                      [(q.dir, q.dir_y) for _, _, q, _ in js], p, u)
        assert np.array_equal(maps[g], one[0])
        assert np.array_equal(cmin[g], one[2]) and np.array_equal(csec[g], one[3])
        if u:
            assert (maps[g] == 0xFFFF).any() and (maps[g] != 0xFFFF).any()
        exp, _ = oracle.fuse_depth(maps[g][None], [js[0][3]], F, PS)
        assert np.array_equal(depth[g].view(np.uint64), exp.view(np.uint64))
        assert (depth[g][maps[g] == 0xFFFF] == 0).all() and (depth[g] > 0).any()


@pytest.mark.parametrize("mode", ["rccl_all", "peer"])
def test_array_depth_mb(ctx, sva, oracle, mode):
    r = rig()
    m = sva.Multi([0], streams=2, flags=FLAGS[mode](sva))
    try:
        res = m.array_depth_mb(r["views"], r["jobs"], r["gs"], F, PS, 10, want_maps=True,
                               want_costs=True)
        again = m.array_depth_mb(r["views"], r["jobs"], r["gs"], F, PS, 10, want_maps=True)
    finally:
        m.close()
    check_array(sva, ctx, oracle, res, 10)
    assert np.array_equal(again[0], res[0]) and np.array_equal(again[1], res[1])
    assert again[2] is None and again[3] is None


def test_array_depth_mb_refusals(sva):
    r = rig()
    v, jobs, gs = r["views"], r["jobs"], r["gs"]
    m = sva.Multi([0], streams=1, flags=sva.SVA_MULTI_GATHER_PEER)

    def changed(j, **kw):
        out = list(jobs)
        a, b, p, base = out[j]
        q = sva.default_params(D=p.D, dir=p.dir, dir_y=p.dir_y)
        for k, val in kw.items():
            if k not in ("ref", "baseline"):
                setattr(q, k, val)
        out[j] = (kw.get("ref", a), b, q, kw.get("baseline", base))
        return out

    INV, UNS = sva.SVA_ERR_INVALID_ARG, sva.SVA_ERR_UNSUPPORTED
    cases = [(changed(2, ref=1), INV), (changed(9, D=40), INV), (changed(3, dmin=1), INV),
             (changed(1, P1=11), INV), (changed(1, P2=100), INV), (changed(10, invalid=0), INV),
             (changed(5, baseline=2 * PITCH_M), INV),
             (changed(5, baseline=PITCH_M * (1 + 1e-6)), INV), (changed(4, lr_check=1), UNS)]
    try:
        for i, (js, status) in enumerate(cases):
            with pytest.raises(sva.SvaError) as e:
                m.array_depth_mb(v, js, gs, F, PS)
            assert e.value.status == status, i
        with pytest.raises(sva.SvaError) as e:
            m.array_depth_mb(v, jobs, gs, F, PS, uniqueness=101)
        assert e.value.status == INV
        # a baseline within 1e-9 relative is the same depth scale
        m.array_depth_mb(v, changed(5, baseline=PITCH_M * (1 + 1e-12)), gs, F, PS)
        c0 = m.context(0, 0)
        c0.set_timing(sva.SVA_TIMING_ALL)
        c0.reset_timing()
        with pytest.raises(sva.SvaError):
            m.array_depth_mb(v, cases[0][0], gs, F, PS)
        assert counts_of(c0) == dict.fromkeys(COUNTED, 0)
    finally:
        m.close()


def test_array_depth_mb_across_devices(ctx, sva, oracle):
    n = min(sva.device_count(), 4)
    if n < 2:
        pytest.skip("needs >= 2 HIP devices")
    r = rig()
    m = sva.Multi(list(range(n)), streams=2, flags=FLAGS["rccl"](sva))
    try:
        res = m.array_depth_mb(r["views"], r["jobs"], r["gs"], F, PS, 10, want_maps=True,
                               want_costs=True)
    finally:
        m.close()
    check_array(sva, ctx, oracle, res, 10)
