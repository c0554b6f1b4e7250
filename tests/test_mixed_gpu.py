"""Mixed-baseline Mode S on the GPU.

Bars: the cost stage bit-exact against mixed_expect.cost on random census
words; the fusion stage bit-exact against mixed_expect.fuse on random volumes;
the frame route's disparity and cost planes bit-exact against mixed_expect ->
oracle.aggregate -> oracle.wta / conf_expect.conf_planes, sub-pixel within the
project's 1e-5; a frame with a known answer; the equivalences of §2.2d byte for
byte; the launches counted by the event timers; every refusal without a launch;
the array route equal to the single-context route and its depth bit-exact
against oracle.fuse_depth on the unit baseline."""
import ctypes as ct
import functools

import numpy as np
import pytest
import torch

from stereovisionarray_amd import synth

import conf_expect as ce
import mixed_expect as mx
from test_array_gpu import SPLIT_STEPS
from test_multibaseline_gpu import stage_volumes, SW, SH

pytestmark = pytest.mark.gpu

SUB_TOL = 1e-5
COUNTED = ("census", "cost", "cost_mixed", "cost_fuse", "sgm_paths", "wta_hv")
# the step and ratio lists of test_mixed_cpu, paired up so that every step and
# every ratio appears, 1-D, diagonal and skew steps at ratios above and below one
STAGE_PAIRS = [((1, 0), (2, 1)), ((-1, 0), (1, 2)), ((0, 1), (3, 1)), ((1, 1), (2, 3)),
               ((2, -1), (3, 2)), ((-1, 3), (7, 8)), ((-3, -2), (8, 1)), ((1, 0), (1, 8)),
               ((2, -1), (1, 1))]
SIZES = [(37, 23), (131, 75)]


def counts_of(ctx):
    return {k: ctx.kernel_time(k)[1] for k in COUNTED}


# ---- the cost stage -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def census_words(W, H):
    """Two maps of uniformly random census words (bits 0..61), read-only."""
    rng = np.random.default_rng(6000 + W)
    a = rng.integers(0, 1 << 62, size=(2, H, W), dtype=np.uint64)
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("D", [64, 128, 192, 256])
def test_cost_mixed_stage(ctx, torch_dev, D, W, H):
    cl, cr = census_words(W, H)
    dl = torch.from_numpy(cl.view(np.int64).copy()).to(torch_dev)
    dr = torch.from_numpy(cr.view(np.int64).copy()).to(torch_dev)
    out = torch.zeros((H, W, D), dtype=torch.uint8, device=torch_dev)
    outside = False
    for dmin in (0, 9):
        for (sx, sy), (num, den) in STAGE_PAIRS:
            exp = mx.cost(cl, cr, D, dmin, sx, sy, num, den)
            outside |= bool((~mx.inside(W, H, D, dmin, sx, sy, num, den)).any())
            for dreal in (D, D - 37):
                e = exp.copy()
                e[:, :, dreal:] = mx.PAD
                out.fill_(7)
                ctx.cost_mixed_d(dl.data_ptr(), dr.data_ptr(), W, H, D, dreal, dmin, (sx, sy),
                                 (num, den), out.data_ptr())
                ctx.synchronize()
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                assert np.array_equal(got, e), (dmin, sx, sy, num, den, dreal,
                                                int((got != e).sum()))
    assert outside
    if W < 64:      # narrower than every D: every pixel has outside cells at ratio >= 1
        assert (~mx.inside(W, H, D, 0, 1, 0, 1, 1)).any(axis=2).all()


def test_cost_mixed_stage_takes_unreduced_ratios(ctx, torch_dev):
    (W, H), D = SIZES[0], 64
    cl, cr = census_words(W, H)
    dl = torch.from_numpy(cl.view(np.int64).copy()).to(torch_dev)
    dr = torch.from_numpy(cr.view(np.int64).copy()).to(torch_dev)
    out = torch.zeros((H, W, D), dtype=torch.uint8, device=torch_dev)
    ctx.cost_mixed_d(dl.data_ptr(), dr.data_ptr(), W, H, D, D, 0, (2, -1), (6, 4), out.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), mx.cost(cl, cr, D, 0, 2, -1, 3, 2))


# ---- the fusion stage ---------------------------------------------------------
def stage_pairs(n):
    p = [STAGE_PAIRS[i % len(STAGE_PAIRS)] for i in range(n)]
    return [s for s, _ in p], [r for _, r in p]


def run_fuse(ctx, dev, vols, stride, steps, ratios, D, dreal, dmin):
    out = torch.zeros((SH, SW, D), dtype=torch.uint8, device=dev)
    ctx.cost_fuse_mixed_d(vols.data_ptr(), stride, steps, ratios, SW, SH, D, dreal, dmin,
                          out.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("N", [1, 3, 8, 17, 32])
@pytest.mark.parametrize("D", [64, 128, 192, 256])
def test_cost_fuse_mixed_stage(ctx, torch_dev, D, N):
    V = stage_volumes(D)[:N]
    steps, ratios = stage_pairs(N)
    vols = torch.from_numpy(V.copy()).to(torch_dev)
    for dmin in (0, 9):
        cnt = mx.counts(SW, SH, D, dmin, steps, ratios)
        # no pair, some pairs; all pairs only from dmin = 0 (at 8/1 the distance
        # of disparity 9 is past the frame)
        assert (cnt == 0).any() and ((cnt == N).any() or dmin)
        if N > 1:
            assert ((cnt > 0) & (cnt < N)).any()
        for dreal in (D, D - 37):
            exp = mx.fuse(list(V), steps, ratios, dmin, dreal)
            got = run_fuse(ctx, torch_dev, vols, SH * SW * D, steps, ratios, D, dreal, dmin)
            assert np.array_equal(got, exp), (dmin, dreal, int((got != exp).sum()))


def test_cost_fuse_mixed_stage_stride_larger_than_volume(ctx, torch_dev):
    D, N, dmin, dreal = 128, 5, 9, 100
    V = stage_volumes(D)[:N]
    nv = SH * SW * D
    stride = nv + 4096 + 48
    buf = np.random.default_rng(5).integers(0, 256, size=stride * N, dtype=np.uint8)
    for i in range(N):
        buf[i * stride:i * stride + nv] = V[i].ravel()
    steps, ratios = stage_pairs(N)
    got = run_fuse(ctx, torch_dev, torch.from_numpy(buf).to(torch_dev), stride, steps, ratios, D,
                   dreal, dmin)
    assert np.array_equal(got, mx.fuse(list(V), steps, ratios, dmin, dreal))


def test_cost_fuse_mixed_at_unit_ratios_equals_cost_fuse(ctx, torch_dev):
    D, N = 64, 8
    V = stage_volumes(D)[:N]
    steps, _ = stage_pairs(N)
    vols = torch.from_numpy(V.copy()).to(torch_dev)
    out = torch.zeros((SH, SW, D), dtype=torch.uint8, device=torch_dev)
    ctx.cost_fuse_d(vols.data_ptr(), SH * SW * D, steps, SW, SH, D, D - 3, 9, out.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    got = run_fuse(ctx, torch_dev, vols, SH * SW * D, steps, [(3, 3)] * N, D, D - 3, 9)
    assert got.tobytes() == out.cpu().numpy().tobytes()


# ---- frame route --------------------------------------------------------------
def _grid5():
    return [(i % 5 - 2, i // 5 - 2) for i in range(25)]


ALL24 = [i for i in range(25) if i != 12]
# name -> (W, H, D, dmin, grid, reference camera, matched cameras, unit k, per-unit disparity)
FRAMES = {
    # the 5x5 rig's centre against all 24: the inner 8 at k = 1, the outer ring at k = 2
    "c24_short": (96, 80, 64, 0, _grid5(), 12, ALL24, 1, 7),
    "c24_long": (96, 80, 64, 0, _grid5(), 12, ALL24, 2, 7),
    # a padded width; k = 1, 2, 2, 2 over the unit 2
    "d40_padded": (131, 75, 40, 2, [(0, 0), (1, 0), (2, 0), (0, 2), (2, 1)], 0, [1, 2, 3, 4], 2,
                   None),
    # major components 2 and 3, a (3, 1) step: ratios 2/3 and 1/1, then 1/1 and 3/2
    "k23_unit3": (96, 80, 64, 0, [(0, 0), (2, 0), (3, 1), (-2, 2), (0, -3), (1, 2)], 0,
                  [1, 2, 3, 4, 5], 3, None),
    "k23_unit2": (96, 80, 64, 0, [(0, 0), (2, 0), (3, 1), (-2, 2), (0, -3), (1, 2)], 0,
                  [1, 2, 3, 4, 5], 2, None),
    # a unit pair on the split cost route -- step (1, 3), whose census_pair
    # writes both census maps -- between pairs at 2/3 and 1/3
    "split_unit": (96, 80, 64, 0, [(0, 0), (2, 0), (-1, -3), (0, 1), (3, -1)], 0, [1, 2, 3, 4], 3,
                   None),
}


@functools.lru_cache(maxsize=None)
def frame(name):
    """Views, steps, ratios and the expected planes of one frame, computed once."""
    import pyoracle as oracle
    W, H, D, dmin, grid, r, others, unit, const = FRAMES[name]
    steps, ratios, kmax = [], [], 0
    for j in others:
        sx, sy, k = synth.pair_step(grid[r], grid[j])
        steps.append((sx, sy))
        ratios.append(mx.reduced(k, unit))
        kmax = max(kmax, k)
    if const is None:      # every pair's match distance stays below D
        delta = synth.array_delta(H, W, max(5, min((D - 1 - dmin) // kmax, 14)))
    else:
        delta = np.full((H, W), const, np.int64)
    views = synth.array_views(H, W, grid, delta, seed=11)
    cen = [oracle.census(v) for v in views]
    Cs = [mx.cost(cen[r], cen[j], D, dmin, sx, sy, n, d)
          for j, (sx, sy), (n, d) in zip(others, steps, ratios)]
    Cf = mx.fuse(Cs, steps, ratios, dmin)
    S = oracle.aggregate(Cf, threads=8)
    disp, sub = oracle.wta(S, dmin, subpixel=True)
    ds, cmin, csec = ce.conf_planes(S)
    assert np.array_equal(disp, (ds + dmin).astype(np.uint16))
    for a in (Cf, disp, sub, cmin, csec):
        a.setflags(write=False)
    return dict(W=W, H=H, D=D, dmin=dmin, ref=views[r], others=[views[j] for j in others],
                steps=steps, ratios=ratios, disp=disp, sub=sub, cmin=cmin, csec=csec)


def test_frames_cover_the_cases(oracle):
    assert sorted(set(frame("c24_short")["ratios"])) == [(1, 1), (2, 1)]
    assert sorted(set(frame("c24_long")["ratios"])) == [(1, 1), (1, 2)]
    assert (2, 3) in frame("k23_unit3")["ratios"] and (3, 2) in frame("k23_unit2")["ratios"]
    assert any(abs(sx) == 3 and abs(sy) == 1 for sx, sy in frame("k23_unit3")["steps"])
    f = frame("split_unit")
    i = [s in SPLIT_STEPS for s in f["steps"]].index(True)
    assert f["ratios"][i] == (1, 1) and 0 < i < len(f["steps"]) - 1
    assert f["ratios"][i - 1] != (1, 1) and f["ratios"][i + 1] != (1, 1)
    for name in FRAMES:
        f = frame(name)
        cnt = mx.counts(f["W"], f["H"], f["D"], f["dmin"], f["steps"], f["ratios"])
        assert ((cnt > 0) & (cnt < len(f["steps"]))).any(), name
    # the helper's cost at ratio 1/1 is the oracle's
    f = frame("c24_short")
    cr, co = oracle.census(f["ref"]), oracle.census(f["others"][3])
    sx, sy = f["steps"][3]
    assert np.array_equal(mx.cost(cr, co, 64, 0, sx, sy, 1, 1), oracle.cost2(cr, co, 64, 0, sx, sy))


@pytest.mark.parametrize("u", [0, 10])
@pytest.mark.parametrize("name", list(FRAMES))
def test_frame_route(ctx, sva, name, u):
    f = frame(name)
    p = sva.default_params(D=f["D"], dmin=f["dmin"], dir=0, dir_y=0, subpixel=1)
    disp, sub, cmin, csec = ctx.disparity_sgm_mixed(f["ref"], f["others"], f["steps"], f["ratios"],
                                                    p, u)
    assert np.array_equal(cmin, f["cmin"])
    assert np.array_equal(csec, f["csec"])
    rej = ce.rejected(f["cmin"], f["csec"], u)
    edisp, esub = ce.apply_filter(f["disp"], f["sub"], rej)
    assert np.array_equal(disp, edisp)
    assert np.array_equal(np.isnan(sub), rej)
    assert np.max(np.abs(sub[~rej] - esub[~rej])) <= SUB_TOL
    if not u:
        assert not rej.any()


@pytest.mark.parametrize("name,answer", [("c24_short", 7), ("c24_long", 14)])
def test_known_answer(ctx, sva, name, answer):
    """A constant per-grid-unit disparity of 7: all 24 pairs fused find it on
    every interior pixel, in units of the short or of the long baseline."""
    f = frame(name)
    p = sva.default_params(D=f["D"], dmin=f["dmin"])
    disp = ctx.disparity_sgm_mixed(f["ref"], f["others"], f["steps"], f["ratios"], p, 0)[0]
    assert (disp[8:-8, 8:-8] == answer).all()
    assert (f["disp"][8:-8, 8:-8] == answer).all()


def test_device_entry_point_plain_instance(ctx, sva):
    """No plane and no uniqueness, device images: the plain WTA instance, the same map."""
    f = frame("k23_unit3")
    p = sva.default_params(D=f["D"], dmin=f["dmin"], subpixel=0)
    W, H = f["W"], f["H"]
    dev = torch.device("cuda:0")
    imgs = [torch.from_numpy(a).to(dev) for a in [f["ref"]] + f["others"]]
    disp = torch.zeros((H, W), dtype=torch.int16, device=dev)
    ctx.disparity_sgm_mixed_d(imgs[0].data_ptr(), [t.data_ptr() for t in imgs[1:]], f["steps"],
                              f["ratios"], W, H, W, p, 0, disp.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(disp.cpu().numpy().view(np.uint16), f["disp"])


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_unit_ratios_equal_the_multi_route(ctx, sva):
    f = frame("c24_short")
    inner = [i for i, r in enumerate(f["ratios"]) if r == (1, 1)]
    assert len(inner) == 8
    oth, st = [f["others"][i] for i in inner], [f["steps"][i] for i in inner]
    p = sva.default_params(D=f["D"], dmin=f["dmin"], subpixel=1)
    assert same(ctx.disparity_sgm_mixed(f["ref"], oth, st, [(1, 1)] * 8, p, 10),
                ctx.disparity_sgm_multi(f["ref"], oth, st, p, 10))


def test_unreduced_ratios_equal_their_reduced_forms(ctx, sva):
    f = frame("c24_short")
    p = sva.default_params(D=f["D"], dmin=f["dmin"], subpixel=1)
    base = ctx.disparity_sgm_mixed(f["ref"], f["others"], f["steps"], f["ratios"], p, 10)
    twice = [(2 * n, 2 * d) for n, d in f["ratios"]]
    assert (2, 2) in twice and (4, 2) in twice
    assert same(base, ctx.disparity_sgm_mixed(f["ref"], f["others"], f["steps"], twice, p, 10))


def test_pair_order_does_not_matter(ctx, sva):
    f = frame("split_unit")
    p = sva.default_params(D=f["D"], dmin=f["dmin"], subpixel=1)
    base = ctx.disparity_sgm_mixed(f["ref"], f["others"], f["steps"], f["ratios"], p, 10)
    for order in ([1, 0, 3, 2], [3, 2, 1, 0], [2, 3, 0, 1]):
        shuf = ctx.disparity_sgm_mixed(f["ref"], [f["others"][i] for i in order],
                                       [f["steps"][i] for i in order],
                                       [f["ratios"][i] for i in order], p, 10)
        assert same(base, shuf), order


def test_one_pair_at_two_to_one(ctx, sva, oracle):
    """n = 1: the fused volume is the pair's own (62 outside is its own value)."""
    f = frame("c24_short")
    i = f["ratios"].index((2, 1))
    sx, sy = f["steps"][i]
    C = mx.cost(oracle.census(f["ref"]), oracle.census(f["others"][i]), f["D"], 0, sx, sy, 2, 1)
    assert np.array_equal(mx.fuse([C], [(sx, sy)], [(2, 1)], 0), C)
    S = oracle.aggregate(C, threads=8)
    edisp, _ = oracle.wta(S, 0, subpixel=False)
    _, cmin, csec = ce.conf_planes(S)
    p = sva.default_params(D=f["D"], dmin=0)
    disp, _, gmin, gsec = ctx.disparity_sgm_mixed(f["ref"], [f["others"][i]], [(sx, sy)], [(2, 1)],
                                                  p, 0)
    assert np.array_equal(disp, edisp)
    assert np.array_equal(gmin, cmin) and np.array_equal(gsec, csec)


def timed(ctx, sva, call):
    ctx.reset_timing()
    ctx.set_timing(sva.SVA_TIMING_ALL)
    try:
        call()
        return counts_of(ctx)
    finally:
        ctx.set_timing(sva.SVA_TIMING_OFF)
        ctx.reset_timing()


def test_kernel_counts(ctx, sva):
    f = frame("c24_short")
    p = sva.default_params(D=f["D"], dmin=f["dmin"])
    got = timed(ctx, sva, lambda: ctx.disparity_sgm_mixed(f["ref"], f["others"], f["steps"],
                                                          f["ratios"], p, 0))
    # the inner 8 on the frame's own cost kernels; one reference census map and
    # one per pair of the outer ring
    assert got == {"census": 17, "cost": 8, "cost_mixed": 16, "cost_fuse": 1, "sgm_paths": 1,
                   "wta_hv": 1}
    inner = [i for i, r in enumerate(f["ratios"]) if r == (1, 1)]
    got = timed(ctx, sva, lambda: ctx.disparity_sgm_mixed(
        f["ref"], [f["others"][i] for i in inner], [f["steps"][i] for i in inner],
        [(5, 5)] * len(inner), p, 0))
    assert got == {"census": 0, "cost": 8, "cost_mixed": 0, "cost_fuse": 1, "sgm_paths": 1,
                   "wta_hv": 1}


def test_refusals_launch_nothing(ctx, sva, torch_dev):
    f = frame("split_unit")
    W, H, D = f["W"], f["H"], f["D"]
    ref, oth, steps, ratios = f["ref"], f["others"], f["steps"], f["ratios"]
    good = sva.default_params(D=D, dmin=f["dmin"])
    lr = sva.default_params(D=D, dmin=f["dmin"], lr_check=1)
    bigd = sva.default_params(D=300)
    badp = sva.default_params(D=D, P2=200)
    far = sva.default_params(D=D, dmin=8200)      # 8 * (8200 + 63) > 65535
    INV, UNS = sva.SVA_ERR_INVALID_ARG, sva.SVA_ERR_UNSUPPORTED

    def mixed(others, st, ra, p, u=0):
        return lambda: ctx.disparity_sgm_mixed(ref, others, st, ra, p, u)

    def with_ratio(r):
        return [ratios[0], r] + ratios[2:]

    def raw_null_image():
        disp = np.zeros((H, W), np.uint16)
        ptrs = (ct.c_void_p * 2)(oth[0].ctypes.data, None)
        st = (ct.c_int32 * 4)(*[v for s in steps[:2] for v in s])
        ra = (ct.c_int32 * 4)(*[v for r in ratios[:2] for v in r])
        ctx._chk(sva.lib.sva_disparity_sgm_mixed(ctx.h, ref.ctypes.data, ptrs, st, ra, 2, W, H, W,
                                                 ct.byref(good), 0, disp.ctypes.data, None, None,
                                                 None))

    cen = torch.zeros((2, H, W), dtype=torch.int64, device=torch_dev)
    vol = torch.zeros((2, H, W, 64), dtype=torch.uint8, device=torch_dev)
    out = torch.zeros((H, W, 64), dtype=torch.uint8, device=torch_dev)
    nv = H * W * 64

    def cost(step=(1, 0), ratio=(2, 1), D=64, dreal=64, dmin=0, a=cen[0], b=cen[1], o=out):
        return lambda: ctx.cost_mixed_d(a.data_ptr() if a is not None else None,
                                        b.data_ptr() if b is not None else None, W, H, D, dreal,
                                        dmin, step, ratio, o.data_ptr() if o is not None else None)

    def fuse(ra=((2, 1), (1, 2)), st=((1, 0), (0, 1)), D=64, dreal=64, stride=nv):
        return lambda: ctx.cost_fuse_mixed_d(vol.data_ptr(), stride, list(st), ra if ra is None
                                             else list(ra), W, H, D, dreal, 0, out.data_ptr())

    cases = [
        (mixed(oth, steps, None, good), INV),                           # null ratios
        (mixed(oth, steps, with_ratio((0, 1)), good), INV),
        (mixed(oth, steps, with_ratio((9, 1)), good), INV),
        (mixed(oth, steps, with_ratio((1, 0)), good), INV),
        (mixed(oth, steps, with_ratio((1, 9)), good), INV),
        (mixed(oth, steps, with_ratio((-2, -1)), good), INV),
        (mixed(oth, steps, with_ratio((8, 1)), far), INV),              # the distance limit
        (mixed([], [], [], good), INV),                                 # n = 0
        (mixed(oth * 9, steps * 9, ratios * 9, good), INV),             # n = 36
        (raw_null_image, INV),
        (mixed(oth, [steps[0], (0, 0)] + steps[2:], ratios, good), INV),
        (mixed(oth, steps, ratios, lr), UNS),
        (mixed(oth, steps, ratios, bigd), UNS),
        (mixed(oth, steps, ratios, badp), INV),
        (mixed(oth, steps, ratios, good, 101), INV),
        (cost(ratio=(0, 1)), INV),
        (cost(ratio=(1, 9)), INV),
        (cost(step=(0, 0)), INV),
        (cost(D=100, dreal=100), UNS),
        (cost(dreal=0), INV),
        (cost(dreal=65), INV),
        (cost(dmin=8200, ratio=(8, 1)), INV),
        (cost(a=None), INV),
        (cost(b=None), INV),
        (cost(o=None), INV),
        (fuse(ra=None), INV),
        (fuse(ra=((2, 1), (0, 2))), INV),
        (fuse(ra=((2, 1), (1, 9))), INV),
        (fuse(st=((1, 0), (0, 0))), INV),
        (fuse(D=100, dreal=100), UNS),
        (fuse(dreal=65), INV),
        (fuse(stride=nv - 16), INV),
        (fuse(stride=nv + 8), INV),
    ]

    def run():
        for i, (call, status) in enumerate(cases):
            with pytest.raises(sva.SvaError) as e:
                call()
            assert e.value.status == status, i

    assert timed(ctx, sva, run) == dict.fromkeys(COUNTED, 0)


# ---- array route --------------------------------------------------------------
AW, AH, AD = 96, 80, 64
PITCH_M, F, PS = 0.05, 0.05, 0.036 / 160


@functools.lru_cache(maxsize=None)
def rig():
    """The 5x5 grid, two groups: the centre against all 24 (unit = the long
    baseline) and corner camera 0 against six cameras at k = 1 and 2 (unit = the
    short one)."""
    import stereovisionarray_amd as sva
    grid = _grid5()
    pairs = [(12, j) for j in ALL24] + [(0, j) for j in (1, 2, 5, 10, 6, 12)]
    views = synth.array_views(AH, AW, grid, synth.array_delta(AH, AW, 14), seed=3)
    jobs, ks = [], []
    for i, j in pairs:
        sx, sy, k = synth.pair_step(grid[i], grid[j])
        jobs.append((i, j, sva.default_params(D=AD, dir=sx, dir_y=sy), k * PITCH_M))
        ks.append(k)
    return dict(views=views, jobs=jobs, ks=ks, gs=[0, 24, 30], unit_k=[2, 1],
                unit=[2 * PITCH_M, PITCH_M])


def test_array_depth_mixed(ctx, sva, oracle):
    r = rig()
    m = sva.Multi([0], streams=2, flags=sva.SVA_MULTI_GATHER_PEER)
    try:
        depth, maps, cmin, csec = m.array_depth_mixed(r["views"], r["jobs"], r["gs"], r["unit"], F,
                                                      PS, 10, want_maps=True, want_costs=True)
        again = m.array_depth_mixed(r["views"], r["jobs"], r["gs"], r["unit"], F, PS, 10,
                                    want_maps=True)
    finally:
        m.close()
    assert np.array_equal(again[0], depth) and np.array_equal(again[1], maps)
    assert again[2] is None and again[3] is None
    for g in range(2):
        lo, hi = r["gs"][g], r["gs"][g + 1]
        js = r["jobs"][lo:hi]
        ratios = [mx.reduced(k, r["unit_k"][g]) for k in r["ks"][lo:hi]]
        assert len(set(ratios)) == 2
        one = ctx.disparity_sgm_mixed(r["views"][js[0][0]], [r["views"][j] for _, j, _, _ in js],
                                      [(q.dir, q.dir_y) for _, _, q, _ in js], ratios,
                                      sva.default_params(D=AD), 10)
        assert np.array_equal(maps[g], one[0])
        assert np.array_equal(cmin[g], one[2]) and np.array_equal(csec[g], one[3])
        assert (maps[g] == 0xFFFF).any() and (maps[g] != 0xFFFF).any()
        exp, _ = oracle.fuse_depth(maps[g][None], [r["unit"][g]], F, PS)
        assert np.array_equal(depth[g].view(np.uint64), exp.view(np.uint64))
        assert (depth[g][maps[g] == 0xFFFF] == 0).all() and (depth[g] > 0).any()


def test_array_depth_mixed_refusals(sva):
    r = rig()
    v, jobs, gs, unit = r["views"], r["jobs"], r["gs"], r["unit"]
    m = sva.Multi([0], streams=1, flags=sva.SVA_MULTI_GATHER_PEER)

    def with_baseline(j, base):
        out = list(jobs)
        out[j] = out[j][:3] + (base,)
        return out

    INV = sva.SVA_ERR_INVALID_ARG
    cases = [(with_baseline(0, unit[0] * (1 + 1e-6)), unit),      # no num/den of the unit
             (with_baseline(3, PITCH_M * (1 + 1e-6)), unit),
             (with_baseline(26, 9 * PITCH_M), unit),              # num = 9
             (with_baseline(3, 0.0), unit),
             (jobs, [2 * PITCH_M, 0.0]),
             (jobs, [2 * PITCH_M, 17 * PITCH_M])]                 # den = 17
    try:
        c0 = m.context(0, 0)
        c0.set_timing(sva.SVA_TIMING_ALL)
        c0.reset_timing()
        for i, (js, ub) in enumerate(cases):
            with pytest.raises(sva.SvaError) as e:
                m.array_depth_mixed(v, js, gs, ub, F, PS)
            assert e.value.status == INV, i
        assert counts_of(c0) == dict.fromkeys(COUNTED, 0)
        # within 1e-9 relative it is that ratio
        a = m.array_depth_mixed(v, with_baseline(3, 2 * PITCH_M * (1 + 1e-12)), gs, unit, F, PS)
        b = m.array_depth_mixed(v, jobs, gs, unit, F, PS)
        assert np.array_equal(a[0], b[0])
        # the equal-baseline route keeps refusing such groups
        with pytest.raises(sva.SvaError) as e:
            m.array_depth_mb(v, jobs, gs, F, PS)
        assert e.value.status == INV
    finally:
        m.close()
