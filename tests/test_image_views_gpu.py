"""Device images as VIEWS: every `_d` entry that takes a pitch, called on a
sub-rectangle of a larger device allocation (tests/views.py) at every residue
of the base address and of the pitch modulo 4, against the CPU oracle on the
contiguous crop.

include/sva.h names no alignment for an image's base or pitch, and the kernels
do depend on the address: sad_row realigns dwords by `addr & 3`, the box
refinement reads through raw buffer offsets r * pitch + q, and several loaders
fetch bytes outside the image that they promise never to use.  So every case
runs with the bytes around the view set to 0x00 and to 0xFF (and, where base
and pitch residue are equal, to random bytes): the results must equal the
oracle at the entry's own bar -- integers bit-exact, sub-pixel within 1e-5 --
AND be bit-identical between the fills, the sub-pixel planes as uint32.  One
byte of a neighbouring row or of the padding that reaches an output shows up as
a difference between two fills.

Several images of one call share `pitch` (the ABI has one per call) and get
different base residues: image i of a call is placed on (base_mod4 + i) % 4.
Outputs that carry a pitch are views too, into parents of random bytes that must
come back unchanged outside the view.  The host entries at the end take a numpy
parent with pitch = W + 13 and a base one byte into a row; those that write a
pitched output must leave the parent unchanged around it.

Not reached here: sad_row inside refine_kernel (k 1..16), which only planes of
2^31 bytes or more take; the refinement cases run the box kernel, the direct
kernel at k = 0 (no window bytes) and the summed-area route, as the asserted
route numbers show.  sad_row at unaligned residues is exercised by Mode R at
k = 33 (sad_span); k <= 32 runs the plane kernel's clamped byte loads."""
import ctypes as ct
import functools

import numpy as np
import pytest
import torch

from stereovisionarray_amd import synth

import conf_expect as ce
import mb_expect
import mixed_expect as mx
import views
from views import ALL16, SUBSET

pytestmark = pytest.mark.gpu

SUB_TOL = 1e-5
INVALID = 0xFFFF
RES = pytest.mark.parametrize("base_mod4,pitch_mod4", ALL16)
RES_SUBSET = pytest.mark.parametrize("base_mod4,pitch_mod4", SUBSET)


# ---- helpers ------------------------------------------------------------------
def fills_for(base_mod4, pitch_mod4):
    """0x00 and 0xFF everywhere; random bytes too on the diagonal of the residue
    table ((1, 1) and (3, 3) of the subset)."""
    return views.FILLS + (("random",) if base_mod4 == pitch_mod4 else ())


class Maker:
    """The views of one call: image i on base residue (base_mod4 + shift) % 4,
    all on one pitch residue and one fill.  Keeps the parents alive."""

    def __init__(self, base_mod4, pitch_mod4, fill, dev):
        self.b, self.p, self.fill, self.dev = base_mod4, pitch_mod4, fill, dev
        self.keep, self.pitch = [], None

    def view(self, img, shift=0, fill=None):
        """(parent tensor, ptr) of a new view."""
        fill = self.fill if fill is None else fill
        t, ptr, pitch = views.make_view(np.asarray(img), (self.b + shift) % 4, self.p, fill,
                                        self.dev, seed=len(self.keep))
        assert self.pitch in (None, pitch)
        self.keep.append(t)
        self.pitch = pitch
        return t, ptr

    def __call__(self, img, shift=0):
        return self.view(img, shift)[1]

    def out(self, init, shift=0):
        """An output view: a parent of random bytes around `init`.  Returns
        (ptr, read); read() fetches the parent, asserts that nothing outside
        the view changed and returns the view's pixels."""
        t, ptr = self.view(init, shift, fill="random")
        before = t.cpu().numpy().copy()
        rect = views.rect_of(t, ptr, t.shape[1], *np.asarray(init).shape)

        def read():
            after = t.cpu().numpy()
            views.assert_outside_unchanged(after, before, rect)
            return views.crop(after, rect).copy()
        return ptr, read


def sync(ctx):
    ctx.synchronize()
    torch.cuda.synchronize()


def bits(a):
    """The array as unsigned integers of its element size (f32 -> uint32)."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def over_fills(base_mod4, pitch_mod4, dev, run):
    """run(Maker) -> tuple of host arrays, once per fill.  Asserts that every
    fill gives bit-identical outputs and returns those of the first."""
    outs = {}
    for fill in fills_for(base_mod4, pitch_mod4):
        outs[fill] = run(Maker(base_mod4, pitch_mod4, fill, dev))
    first = outs[0x00]
    for fill, got in outs.items():
        assert len(got) == len(first)
        for i, (a, b) in enumerate(zip(first, got)):
            assert a.shape == b.shape and a.dtype == b.dtype
            diff = bits(a) != bits(b)
            assert not diff.any(), (f"output {i} depends on the bytes around the view: fill "
                                    f"{fill!r} differs from 0x00 in {int(diff.sum())} elements, "
                                    f"first at {tuple(int(v) for v in np.argwhere(diff)[0])}")
    return first


def zeros(shape, dtype, dev, value=0):
    return torch.full(shape, value, dtype=dtype, device=dev)


def u16(t):
    return t.cpu().numpy().view(np.uint16)


def check_sub(sub, exp, bad):
    """NaN exactly on `bad`, elsewhere within the project's 1e-5 px."""
    assert np.array_equal(np.isnan(sub), bad)
    assert np.max(np.abs(sub[~bad] - exp[~bad]), initial=0.0) <= SUB_TOL


def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


# ---- census_d -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def census_case(W, H):
    import pyoracle as oracle
    img = synth.texture(H, W, W * 31 + H)
    img[::7, ::5] = 128          # equal-valued neighbours: '<' stays strict
    exp = oracle.census(img)
    frozen(img, exp)
    return img, exp


@pytest.mark.parametrize("W,H", [(41, 23), (9, 7)])       # 9x7: one window
@RES
def test_census_d(ctx, torch_dev, base_mod4, pitch_mod4, W, H):
    img, exp = census_case(W, H)
    assert exp.any()

    def run(mk):
        out = zeros((H, W), torch.int64, torch_dev, 0x55)
        ctx.census_d(mk(img), W, H, mk.pitch, out.data_ptr())
        sync(ctx)
        return (out.cpu().numpy().view(np.uint64),)

    got, = over_fills(base_mod4, pitch_mod4, torch_dev, run)
    assert np.array_equal(got, exp)


# ---- census_cost_d ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cost_case(W, H, D, dmin, sx, sy):
    import pyoracle as oracle
    if sy == 0:
        L, R, _ = synth.stereo_pair(H, W, D, dmin, sx, seed=D + dmin)
        exp = oracle.cost(oracle.census(L), oracle.census(R), D, dmin, sx)
    else:
        L, R, _ = synth.stereo_pair2(H, W, D, dmin, sx, sy, seed=D + 3 * sx + sy)
        exp = oracle.cost2(oracle.census(L), oracle.census(R), D, dmin, sx, sy)
    assert (exp == 62).any() and (exp < 62).any()
    frozen(L, R, exp)
    return L, R, exp


def run_census_cost(ctx, sva, dev, base_mod4, pitch_mod4, W, H, D, dmin, sx, sy):
    L, R, exp = cost_case(W, H, D, dmin, sx, sy)
    p = sva.default_params(D=D, dmin=dmin, dir=sx, dir_y=sy)

    def run(mk):
        C = zeros((H, W, D), torch.uint8, dev, 0xAA)
        ctx.census_cost_d(mk(L), mk(R, 1), W, H, mk.pitch, p, C.data_ptr())
        sync(ctx)
        return (C.cpu().numpy(),)

    got, = over_fills(base_mod4, pitch_mod4, dev, run)
    assert np.array_equal(got, exp), (dmin, sx, sy, int((got != exp).sum()))


@pytest.mark.parametrize("D", [64, 128])
@RES
def test_census_cost_d_1d_steps(ctx, sva, torch_dev, base_mod4, pitch_mod4, D):
    """W = 203 leaves a ragged 128-pixel tile."""
    for dir, dmin in ((-1, 0), (1, 0), (-1, 7), (1, 7)):
        run_census_cost(ctx, sva, torch_dev, base_mod4, pitch_mod4, 203, 11, D, dmin, dir, 0)


@pytest.mark.parametrize("sx,sy", [(1, 1), (-2, 1), (0, -1)])
@RES
def test_census_cost_d_2d_steps(ctx, sva, torch_dev, base_mod4, pitch_mod4, sx, sy):
    run_census_cost(ctx, sva, torch_dev, base_mod4, pitch_mod4, 131, 37, 64, 0, sx, sy)


# ---- disparity_sgm_d / disparity_sgm_conf_d -----------------------------------
# name -> (W, H, D, dmin, dir, lr_check)
SGM_CASES = {"70x40_d64": (70, 40, 64, 0, -1, 0), "97x33_d100_lr": (97, 33, 100, 2, 1, 1)}


@functools.lru_cache(maxsize=None)
def sgm_case(name):
    """The pair and everything expected of it: the plain map (with the L/R check
    where the case has one), and the confidence route at uniqueness 10."""
    import pyoracle as oracle
    W, H, D, dmin, dir, lr = SGM_CASES[name]
    L, R, _ = synth.stereo_pair(H, W, D, dmin, dir, seed=W + D, stripes=6, step=9)
    S = oracle.aggregate(oracle.cost(oracle.census(L), oracle.census(R), D, dmin, dir), threads=8)
    disp, sub = oracle.wta(S, dmin, subpixel=True)
    od, osub = oracle.sgm(L, R, D, dmin, dir, subpixel=True, threads=8)
    assert np.array_equal(disp, od) and np.array_equal(bits(sub), bits(osub))
    ds, cmin, csec = ce.conf_planes(S)
    rej = ce.rejected(cmin, csec, 10)
    assert rej.any() and not rej.all()
    conf_disp, _ = ce.apply_filter(disp, None, rej, INVALID)
    if lr:      # the right-referenced pass swaps the images: both views serve both roles
        dr, _ = oracle.sgm(R, L, D, dmin, -dir, subpixel=False, threads=8)
        disp = oracle.lr_check(disp, dr, dir, 1, INVALID)
        conf_disp = oracle.lr_check(conf_disp, dr, dir, 1, INVALID)
        assert (disp == INVALID).any() and ((conf_disp == INVALID) & ~rej).any()
    assert (conf_disp != INVALID).any()
    frozen(L, R, disp, sub, cmin, csec, conf_disp)
    return dict(L=L, R=R, disp=disp, sub=sub, cmin=cmin, csec=csec, conf_disp=conf_disp)


def sgm_params(sva, name):
    W, H, D, dmin, dir, lr = SGM_CASES[name]
    return sva.default_params(D=D, dmin=dmin, dir=dir, subpixel=1, lr_check=lr, lr_max_diff=1,
                              invalid=INVALID)


@pytest.mark.parametrize("name", list(SGM_CASES))
@RES
def test_disparity_sgm_d(ctx, sva, torch_dev, base_mod4, pitch_mod4, name):
    W, H = SGM_CASES[name][:2]
    e = sgm_case(name)
    p = sgm_params(sva, name)

    def run(mk):
        disp = zeros((H, W), torch.int16, torch_dev, 0x5A5A)
        sub = zeros((H, W), torch.float32, torch_dev, 7.0)
        ctx.disparity_sgm_d(mk(e["L"]), mk(e["R"], 1), W, H, mk.pitch, p, disp.data_ptr(),
                            sub.data_ptr())
        sync(ctx)
        return u16(disp), sub.cpu().numpy()

    disp, sub = over_fills(base_mod4, pitch_mod4, torch_dev, run)
    assert np.array_equal(disp, e["disp"])
    check_sub(sub, e["sub"], e["disp"] == INVALID)


@pytest.mark.parametrize("name", list(SGM_CASES))
@RES
def test_disparity_sgm_conf_d(ctx, sva, torch_dev, base_mod4, pitch_mod4, name):
    """Uniqueness 10 and both cost planes."""
    W, H = SGM_CASES[name][:2]
    e = sgm_case(name)
    p = sgm_params(sva, name)

    def run(mk):
        disp, cmin, csec = (zeros((H, W), torch.int16, torch_dev, 0x5A5A) for _ in range(3))
        sub = zeros((H, W), torch.float32, torch_dev, 7.0)
        ctx.disparity_sgm_conf_d(mk(e["L"]), mk(e["R"], 1), W, H, mk.pitch, p, 10,
                                 disp.data_ptr(), sub.data_ptr(), cmin.data_ptr(), csec.data_ptr())
        sync(ctx)
        return u16(disp), sub.cpu().numpy(), u16(cmin), u16(csec)

    disp, sub, cmin, csec = over_fills(base_mod4, pitch_mod4, torch_dev, run)
    assert np.array_equal(cmin, e["cmin"]) and np.array_equal(csec, e["csec"])
    assert np.array_equal(disp, e["conf_disp"])
    check_sub(sub, e["sub"], e["conf_disp"] == INVALID)


# ---- disparity_sgm_multi_d / disparity_sgm_mixed_d ------------------------------
def _group_expect(views_, r, others, Cs, fused, dmin):
    import pyoracle as oracle
    S = oracle.aggregate(fused, threads=8)
    disp, sub = oracle.wta(S, dmin, subpixel=True)
    ds, cmin, csec = ce.conf_planes(S)
    rej = ce.rejected(cmin, csec, 10)
    assert rej.any() and not rej.all()
    disp, sub = ce.apply_filter(disp, sub, rej, INVALID)
    frozen(disp, sub, cmin, csec)
    return dict(ref=views_[r], others=[views_[j] for j in others], disp=disp, sub=sub, cmin=cmin,
                csec=csec, rej=rej)


@functools.lru_cache(maxsize=None)
def multi_case():
    """64x48, D = 64: the centre of a 3x3 rig against its 4 axis neighbours,
    steps (+-1, 0) and (0, +-1); expected values through mb_expect."""
    import pyoracle as oracle
    W, H, D, dmin = 64, 48, 64, 0
    grid = [(i % 3 - 1, i // 3 - 1) for i in range(9)]
    r, others = 4, [1, 3, 5, 7]
    steps = [synth.pair_step(grid[r], grid[j])[:2] for j in others]
    assert sorted(steps) == [(-1, 0), (0, -1), (0, 1), (1, 0)]
    vs = synth.array_views(H, W, grid, synth.array_delta(H, W, 14), seed=11)
    cen = [oracle.census(v) for v in vs]
    Cs = [oracle.cost2(cen[r], cen[j], D, dmin, sx, sy) for j, (sx, sy) in zip(others, steps)]
    cnt = mb_expect.counts(W, H, D, dmin, steps)
    assert ((cnt > 0) & (cnt < len(steps))).any()
    e = _group_expect(vs, r, others, Cs, mb_expect.fuse(Cs, steps, dmin), dmin)
    return dict(e, W=W, H=H, D=D, dmin=dmin, steps=steps)


@functools.lru_cache(maxsize=None)
def mixed_case():
    """64x48, D = 64: 3 pairs at 1/1, 2/1 and 1/2 of the unit baseline (2 grid
    units); expected values through mixed_expect."""
    import pyoracle as oracle
    W, H, D, dmin, unit = 64, 48, 64, 0, 2
    grid = [(0, 0), (2, 0), (0, 4), (-1, 0)]
    r, others = 0, [1, 2, 3]
    steps, ratios = [], []
    for j in others:
        sx, sy, k = synth.pair_step(grid[r], grid[j])
        steps.append((sx, sy))
        ratios.append(mx.reduced(k, unit))
    assert ratios == [(1, 1), (2, 1), (1, 2)]
    vs = synth.array_views(H, W, grid, synth.array_delta(H, W, 7), seed=11)
    cen = [oracle.census(v) for v in vs]
    Cs = [mx.cost(cen[r], cen[j], D, dmin, sx, sy, n, d)
          for j, (sx, sy), (n, d) in zip(others, steps, ratios)]
    cnt = mx.counts(W, H, D, dmin, steps, ratios)
    assert ((cnt > 0) & (cnt < len(steps))).any()
    e = _group_expect(vs, r, others, Cs, mx.fuse(Cs, steps, ratios, dmin), dmin)
    return dict(e, W=W, H=H, D=D, dmin=dmin, steps=steps, ratios=ratios)


def run_group(ctx, sva, dev, base_mod4, pitch_mod4, e, call):
    W, H = e["W"], e["H"]
    p = sva.default_params(D=e["D"], dmin=e["dmin"], dir=0, dir_y=0, subpixel=1, invalid=INVALID)

    def run(mk):
        disp, cmin, csec = (zeros((H, W), torch.int16, dev, 0x5A5A) for _ in range(3))
        sub = zeros((H, W), torch.float32, dev, 7.0)
        # the reference view on base_mod4, every neighbour on another residue
        ref = mk(e["ref"])
        oth = [mk(a, 1 + i % 3) for i, a in enumerate(e["others"])]
        call(ref, oth, W, H, mk.pitch, p, 10, disp.data_ptr(), sub.data_ptr(), cmin.data_ptr(),
             csec.data_ptr())
        sync(ctx)
        return u16(disp), sub.cpu().numpy(), u16(cmin), u16(csec)

    disp, sub, cmin, csec = over_fills(base_mod4, pitch_mod4, dev, run)
    assert np.array_equal(cmin, e["cmin"]) and np.array_equal(csec, e["csec"])
    assert np.array_equal(disp, e["disp"])
    check_sub(sub, e["sub"], e["rej"])


@RES
def test_disparity_sgm_multi_d(ctx, sva, torch_dev, base_mod4, pitch_mod4):
    e = multi_case()
    run_group(ctx, sva, torch_dev, base_mod4, pitch_mod4, e,
              lambda ref, oth, *a: ctx.disparity_sgm_multi_d(ref, oth, e["steps"], *a))


@RES
def test_disparity_sgm_mixed_d(ctx, sva, torch_dev, base_mod4, pitch_mod4):
    e = mixed_case()
    run_group(ctx, sva, torch_dev, base_mod4, pitch_mod4, e,
              lambda ref, oth, *a: ctx.disparity_sgm_mixed_d(ref, oth, e["steps"], e["ratios"],
                                                             *a))


# ---- the batch routes: 3 pairs of 70x40 in ONE parent ---------------------------
BATCH_STEPS = [(-1, 0), (0, 1), (-1, -1)]


@functools.lru_cache(maxsize=None)
def batch_case():
    import pyoracle as oracle
    W, H, D = 70, 40, 64
    out = []
    for i, (sx, sy) in enumerate(BATCH_STEPS):
        if sy == 0:
            L, R, _ = synth.stereo_pair(H, W, D, 0, sx, seed=70 + i, stripes=4, step=5)
        else:
            L, R, _ = synth.stereo_pair2(H, W, D, 0, sx, sy, seed=70 + i, stripes=4, step=5)
        S = oracle.aggregate(oracle.cost2(oracle.census(L), oracle.census(R), D, 0, sx, sy),
                             threads=8)
        disp, sub = oracle.wta(S, 0, subpixel=True)
        od, _ = oracle.sgm2(L, R, D, 0, sx, sy, subpixel=False)
        assert np.array_equal(disp, od)
        ds, cmin, csec = ce.conf_planes(S)
        rej = ce.rejected(cmin, csec, 10)
        assert rej.any() and not rej.all()
        frozen(L, R, disp, sub, cmin, csec, rej)
        out.append(dict(L=L, R=R, disp=disp, sub=sub, cmin=cmin, csec=csec, rej=rej))
    return W, H, D, out


def batch_views(sva, base_mod4, pitch_mod4, fill, dev):
    """The six images in one parent, image i on (base_mod4 + i) % 4."""
    W, H, D, fr = batch_case()
    imgs = [a for f in fr for a in (f["L"], f["R"])]
    t, ptrs, pitch = views.make_views(imgs, [(base_mod4 + i) % 4 for i in range(6)], pitch_mod4,
                                      fill, dev)
    pairs = [(ptrs[2 * i], ptrs[2 * i + 1],
              sva.default_params(D=D, dir=sx, dir_y=sy, subpixel=1, invalid=INVALID))
             for i, (sx, sy) in enumerate(BATCH_STEPS)]
    return t, pairs, pitch


def check_batch(got, conf):
    W, H, D, fr = batch_case()
    maps, sub = got[0], got[1]
    for i, f in enumerate(fr):
        rej = f["rej"] if conf else np.zeros_like(f["rej"])
        exp, _ = ce.apply_filter(f["disp"], None, rej, INVALID)
        assert np.array_equal(maps[i], exp), i
        check_sub(sub[i], f["sub"], rej)
        if conf:
            assert np.array_equal(got[2][i], f["cmin"]) and np.array_equal(got[3][i], f["csec"]), i


@RES
def test_disparity_sgm_batch_d(ctx, sva, torch_dev, base_mod4, pitch_mod4):
    W, H, D, fr = batch_case()

    def run(mk):
        t, pairs, pitch = batch_views(sva, mk.b, mk.p, mk.fill, torch_dev)
        maps = zeros((3, H, W), torch.int16, torch_dev, 0x5A5A)
        sub = zeros((3, H, W), torch.float32, torch_dev, 7.0)
        ctx.disparity_sgm_batch_d(pairs, W, H, pitch, maps.data_ptr(), sub.data_ptr())
        sync(ctx)
        return u16(maps), sub.cpu().numpy()

    check_batch(over_fills(base_mod4, pitch_mod4, torch_dev, run), conf=False)


@RES
def test_disparity_sgm_batch_conf_d(ctx, sva, torch_dev, base_mod4, pitch_mod4):
    W, H, D, fr = batch_case()

    def run(mk):
        t, pairs, pitch = batch_views(sva, mk.b, mk.p, mk.fill, torch_dev)
        maps, cmin, csec = (zeros((3, H, W), torch.int16, torch_dev, 0x5A5A) for _ in range(3))
        sub = zeros((3, H, W), torch.float32, torch_dev, 7.0)
        ctx.disparity_sgm_batch_conf_d(pairs, W, H, pitch, 10, maps.data_ptr(), sub.data_ptr(),
                                       cmin.data_ptr(), csec.data_ptr())
        sync(ctx)
        return u16(maps), sub.cpu().numpy(), u16(cmin), u16(csec)

    check_batch(over_fills(base_mod4, pitch_mod4, torch_dev, run), conf=True)


@pytest.fixture(scope="module")
def engine(sva):
    m = sva.Multi([0], streams=2, flags=sva.SVA_MULTI_GATHER_RCCL)
    yield m
    m.close()


@RES_SUBSET
def test_engine_batch_sgm_d(ctx, sva, engine, torch_dev, base_mod4, pitch_mod4):
    """Multi([0]).batch_sgm_d on the same three pairs."""
    W, H, D, fr = batch_case()

    def run(mk):
        t, pairs, pitch = batch_views(sva, mk.b, mk.p, mk.fill, torch_dev)
        maps = zeros((3, H, W), torch.int16, torch_dev, 0x5A5A)
        sub = zeros((3, H, W), torch.float32, torch_dev, 7.0)
        torch.cuda.synchronize()
        engine.batch_sgm_d(pairs, W, H, pitch, maps.data_ptr(), sub.data_ptr())
        engine.synchronize()
        return u16(maps), sub.cpu().numpy()

    check_batch(over_fills(base_mod4, pitch_mod4, torch_dev, run), conf=False)


# ---- disparity_ref_d (Mode R) ---------------------------------------------------
# rig pairs with a horizontal, a vertical and a diagonal line
REF_PAIRS = [(12, 11), (12, 7), (12, 6)]
REF_K = [1, 2, 5, 16, 17, 20]    # both values of 2k % 4, the last sad_row instance, the plane
#                                  route on either side of its switch
INIT8, INIT16 = 77, 777


def ref_cams(sva, W, a, b):
    import pyoracle as oracle
    grid = synth.reference_array(0.036 / W)
    return (sva.Camera.make(*grid[a]), sva.Camera.make(*grid[b]),
            oracle.OCamera.make(*grid[a]), oracle.OCamera.make(*grid[b]))


@functools.lru_cache(maxsize=None)
def ref_case(W, H, k, pair, masked):
    """Images, the dense mask (sva.h: W*H u8, it has no pitch) and oracle.ref_pair's
    planes on outputs preset to 77 / 777 / 0."""
    import pyoracle as oracle
    import stereovisionarray_amd as sva
    _, _, ocr, oco = ref_cams(sva, W, *pair)
    a = synth.texture(H, W, 10 * k + pair[1])
    gx, gy = pair[1] % 5 - 2, pair[1] // 5 - 2
    b = np.roll(np.roll(a, -(W // 8) * gy, axis=0), -(W // 8) * gx, axis=1)
    b = np.ascontiguousarray(b)
    mask = None
    if masked:
        mask = (np.random.default_rng(k + pair[1]).random((H, W)) < 0.7).astype(np.uint8)
    o8 = np.full((H, W), INIT8, np.uint8)
    o16 = np.full((H, W), INIT16, np.uint16)
    ov = np.zeros((H, W), np.uint8)
    _, _, _, n = oracle.ref_pair(a, b, ocr, oco, k=k, mask=mask, disp_u8=o8, disp_u16=o16,
                                 valid=ov)
    assert n > 0 and ov.sum() > 0 and (o16[ov == 1] != INIT16).any()
    frozen(a, b, mask, o8, o16, ov)
    return a, b, mask, o8, o16, ov


def run_ref(ctx, sva, dev, base_mod4, pitch_mod4, W, H, k, pair, masked):
    a, b, mask, o8, o16, ov = ref_case(W, H, k, pair, masked)
    cr, co, _, _ = ref_cams(sva, W, *pair)
    dmask = None if mask is None else torch.from_numpy(np.array(mask)).to(dev)

    def run(mk):
        d8 = zeros((H, W), torch.uint8, dev, INIT8)
        d16 = zeros((H, W), torch.int16, dev, INIT16)
        val = zeros((H, W), torch.uint8, dev, 0)
        ctx.disparity_ref_d(mk(a), mk(b, 1), W, H, mk.pitch,
                            None if dmask is None else dmask.data_ptr(), cr, co, k, 0.5, 1.0,
                            d8.data_ptr(), d16.data_ptr(), val.data_ptr())
        sync(ctx)
        return d8.cpu().numpy(), u16(d16), val.cpu().numpy()

    d8, d16, val = over_fills(base_mod4, pitch_mod4, dev, run)
    what = (k, pair, masked)
    assert np.array_equal(val, ov), what
    assert np.array_equal(d16, o16), (what, int((d16 != o16).sum()))
    assert np.array_equal(d8, o8), what


@pytest.mark.parametrize("k", REF_K)
@RES
def test_disparity_ref_d(ctx, sva, torch_dev, base_mod4, pitch_mod4, k):
    for pair in REF_PAIRS:
        run_ref(ctx, sva, torch_dev, base_mod4, pitch_mod4, 96, 64, k, pair, False)


@pytest.mark.parametrize("k", REF_K)
@RES_SUBSET
def test_disparity_ref_d_masked(ctx, sva, torch_dev, base_mod4, pitch_mod4, k):
    for pair in REF_PAIRS:
        run_ref(ctx, sva, torch_dev, base_mod4, pitch_mod4, 96, 64, k, pair, True)


@pytest.mark.parametrize("masked", [False, True])
@RES_SUBSET
def test_disparity_ref_d_k33_sad_span(ctx, sva, torch_dev, base_mod4, pitch_mod4, masked):
    """k = 33: rows of 66 bytes through sad_span, one 64-byte piece and a rest."""
    for pair in REF_PAIRS:
        run_ref(ctx, sva, torch_dev, base_mod4, pitch_mod4, 120, 104, 33, pair, masked)


# ---- shift_perspective_d --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shift_case(b):
    import pyoracle as oracle
    import stereovisionarray_amd as sva
    W, H = 173, 91
    _, _, oi, oo = ref_cams(sva, W, 12, b)
    rng = np.random.default_rng(b)
    disp = rng.integers(0, 60, size=(H, W)).astype(np.uint8)
    disp[rng.random((H, W)) < 0.1] = 0
    img = synth.texture(H, W, b)
    init = rng.integers(0, 256, size=(H, W)).astype(np.uint8)
    exp = oracle.shift_perspective(oi, oo, disp, img, init=init)
    assert (exp == init).any() and (exp != init).any()
    frozen(disp, img, init, exp)
    return W, H, disp, img, init, exp


@pytest.mark.parametrize("b", [11, 6])
@RES
def test_shift_perspective_d(ctx, sva, torch_dev, base_mod4, pitch_mod4, b):
    """All three planes share the pitch; `shifted` is a view into random bytes:
    inside it equals the oracle started from that prefill, outside nothing changes."""
    W, H, disp, img, init, exp = shift_case(b)
    ci, co, _, _ = ref_cams(sva, W, 12, b)

    def run(mk):
        d, i = mk(disp), mk(img, 1)
        out, read = mk.out(init, 2)
        ctx._chk(sva.lib.sva_shift_perspective_d(ctx.h, ct.byref(ci), ct.byref(co), d, i, W, H,
                                                 mk.pitch, out))
        sync(ctx)
        return (read(),)

    got, = over_fills(base_mod4, pitch_mod4, torch_dev, run)
    assert np.array_equal(got, exp)


# ---- improve_with_disparity_d ---------------------------------------------------
# window -> k = (window - 1) / 2: 1 -> 0 the direct kernel; 7, 32 and 33 -> 3, 15
# and 16 the box kernel (16 is its last size); 35 -> 17 the summed-area route
WINDOWS = [1, 7, 32, 33, 35]


@functools.lru_cache(maxsize=None)
def refine_case(window, share):
    import pyoracle as oracle
    import stereovisionarray_amd as sva
    W, H = 150, 110
    rng = np.random.default_rng(1000 * window + int(100 * share))
    center = synth.texture(H, W, 3)
    opairs, imgs = [], []
    for i, b in enumerate((13, 7, 18, 6)):     # horizontal, vertical and two diagonal steps
        _, _, oi, oo = ref_cams(sva, W, 12, b)
        opairs.append((oi, oo))
        imgs.append(synth.texture(H, W, 60 + i))
    disp = rng.integers(0, 12, size=(H, W)).astype(np.uint8)
    mask = (rng.random((H, W)) < share).astype(np.uint8)
    init = rng.integers(0, 256, size=(H, W)).astype(np.uint8)
    st, exp = oracle.improve_with_disparity(disp, center, imgs, opairs, window=window, mask=mask,
                                            init=init)
    assert st == 0 and (exp != init).any() and (exp == init).any()
    frozen(center, disp, mask, init, exp, *imgs)
    return W, H, center, imgs, disp, mask, init, exp


@pytest.mark.parametrize("window", WINDOWS)
@RES
def test_improve_with_disparity_d(ctx, sva, torch_dev, base_mod4, pitch_mod4, window):
    """Every u8 plane of the call is a view on its own base residue: disparity,
    centre, the 4 images, the mask and the output (unchanged outside).  A 70 %
    and a 2 % mask."""
    want = {1: 1, 7: 0, 32: 0, 33: 0, 35: 2}[window]
    for share in (0.7, 0.02):
        W, H, center, imgs, disp, mask, init, exp = refine_case(window, share)
        pairs = [ref_cams(sva, W, 12, b)[:2] for b in (13, 7, 18, 6)]

        def run(mk):
            d, c = mk(disp), mk(center, 1)
            im = [mk(a, 2 + i) for i, a in enumerate(imgs)]
            m = mk(mask, 6)
            out, read = mk.out(init, 7)
            ctx.improve_with_disparity_d(d, c, im, pairs, W, H, mk.pitch, m, window, False, out)
            sync(ctx)
            assert ctx.get_debug(sva.SVA_DEBUG_REFINE_LAST_ROUTE) == want
            return (read(),)

        got, = over_fills(base_mod4, pitch_mod4, torch_dev, run)
        assert np.array_equal(got, exp), (window, share, int((got != exp).sum()))


# ---- resize_half_d --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def resize_case(W, H):
    import pyoracle as oracle
    img = synth.texture(H, W, W + H)
    exp = oracle.resize_half(img)
    frozen(img, exp)
    return img, exp


@pytest.mark.parametrize("W,H", [(301, 77), (5, 7)])
@RES
def test_resize_half_d(ctx, sva, torch_dev, base_mod4, pitch_mod4, W, H):
    """Source and destination are views; the destination takes every pitch
    residue and keeps its surroundings."""
    img, exp = resize_case(W, H)
    dw, dh = sva.resize_half_size(W, H)
    assert exp.shape == (dh, dw)
    init = np.full((dh, dw), 7, np.uint8)
    for dst_mod4 in range(4):
        def run(mk):
            src = mk(img)
            dst = Maker((mk.b + 1 + dst_mod4) % 4, dst_mod4, "random", torch_dev)
            ptr, read = dst.out(init)
            assert dst.pitch % 4 == dst_mod4
            ctx.resize_half_d(src, W, H, mk.pitch, ptr, dst.pitch)
            sync(ctx)
            return (read(),)

        got, = over_fills(base_mod4, pitch_mod4, torch_dev, run)
        assert np.array_equal(got, exp), dst_mod4


# ---- host entries: a numpy parent, pitch = W + 13, base one byte into a row -----
def host_view(img, seed):
    """(parent, address, pitch) of a host view of img: random bytes around it."""
    H, W = img.shape
    pitch = W + 13
    parent = np.random.default_rng(seed).integers(0, 256, size=(H + 2, pitch), dtype=np.uint8)
    parent[1:H + 1, 1:W + 1] = img
    return parent, parent.ctypes.data + pitch + 1, pitch


def test_host_disparity_sgm_pitched(ctx, sva):
    """sva_disparity_sgm's 2-D upload (hipMemcpy2DAsync in sva_api.cpp)."""
    W, H, D = 97, 33, 64
    L, R, _ = synth.stereo_pair(H, W, D, 0, -1, seed=4)
    p = sva.default_params(D=D, subpixel=1)
    ed, es = ctx.disparity_sgm(L, R, p)
    (pl, al, pitch), (pr, ar, _) = host_view(L, 1), host_view(R, 2)
    disp, sub = np.zeros((H, W), np.uint16), np.zeros((H, W), np.float32)
    ctx._chk(sva.lib.sva_disparity_sgm(ctx.h, al, ar, W, H, pitch, ct.byref(p), disp.ctypes.data,
                                       sub.ctypes.data))
    assert np.array_equal(disp, ed) and np.array_equal(bits(sub), bits(es))
    assert len(np.unique(ed)) > 4


def test_host_disparity_sgm_multi_pitched(ctx, sva):
    """sva_disparity_sgm_multi: the second 2-D copy, the matched images'."""
    e = multi_case()
    W, H = e["W"], e["H"]
    p = sva.default_params(D=e["D"], dmin=e["dmin"], subpixel=1, invalid=INVALID)
    want = ctx.disparity_sgm_multi(e["ref"], e["others"], e["steps"], p, 10)
    hv = [host_view(a, 10 + i) for i, a in enumerate([e["ref"]] + e["others"])]
    pitch = hv[0][2]
    disp, cmin, csec = (np.zeros((H, W), np.uint16) for _ in range(3))
    sub = np.zeros((H, W), np.float32)
    ctx._sgm_multi_d(sva.lib.sva_disparity_sgm_multi, hv[0][1], [v[1] for v in hv[1:]], e["steps"],
                     (), W, H, pitch, p, 10, disp, sub, cmin, csec)
    for got, exp in zip((disp, sub, cmin, csec), want):
        assert np.array_equal(bits(got), bits(exp))
    assert np.array_equal(disp, e["disp"])


def host_out(init, seed):
    """A host OUTPUT view of init in random bytes: (address, pitch, read); read()
    asserts that no byte outside the view changed and returns the view's pixels."""
    parent, addr, pitch = host_view(init, seed)
    before = parent.copy()
    rect = (1, 1) + init.shape

    def read():
        views.assert_outside_unchanged(parent, before, rect)
        return views.crop(parent, rect).copy()
    return addr, pitch, read


def test_host_resize_half_pitched_dst(ctx, sva):
    """sva_resize_half into a destination inside a larger host image: only the
    pixels come back, the bytes between the destination's rows keep their
    values (sva.h, Conventions)."""
    W, H = 301, 77
    img, exp = resize_case(W, H)
    dw, dh = sva.resize_half_size(W, H)
    keep, src, pitch = host_view(img, 30)
    # something else in the context's output staging buffer first
    ctx.resize_half(synth.texture(2 * dh + 40, 2 * dw + 40, 1))
    dst, dst_pitch, read = host_out(np.full((dh, dw), 7, np.uint8), 31)
    ctx._chk(sva.lib.sva_resize_half(ctx.h, src, W, H, pitch, dst, dst_pitch))
    assert np.array_equal(read(), exp)


def test_host_shift_perspective_pitched(ctx, sva):
    """sva_shift_perspective: the output plane goes up and comes back whole."""
    W, H, disp, img, init, exp = shift_case(11)
    ci, co, _, _ = ref_cams(sva, W, 12, 11)
    (k1, d, pitch), (k2, i, _) = host_view(disp, 40), host_view(img, 41)
    out, _, read = host_out(init, 42)
    ctx._chk(sva.lib.sva_shift_perspective(ctx.h, ct.byref(ci), ct.byref(co), d, i, W, H, pitch,
                                           out))
    assert np.array_equal(read(), exp)


def test_host_improve_with_disparity_pitched(ctx, sva):
    """sva_improve_with_disparity (window 7, the box kernel): every plane a host
    view, the output unchanged outside."""
    W, H, center, imgs, disp, mask, init, exp = refine_case(7, 0.7)
    hv = [host_view(a, 50 + n) for n, a in enumerate([disp, center, mask] + list(imgs))]
    pitch = hv[0][2]
    out, _, read = host_out(init, 60)
    cams = (sva.Camera * 8)()
    for n, b in enumerate((13, 7, 18, 6)):
        cams[2 * n], cams[2 * n + 1] = ref_cams(sva, W, 12, b)[:2]
    ptrs = (ct.c_void_p * 4)(*[v[1] for v in hv[3:]])
    ctx._chk(sva.lib.sva_improve_with_disparity(ctx.h, hv[0][1], hv[1][1], ptrs, cams, 4, W, H,
                                                pitch, hv[2][1], 7, 0, out))
    assert np.array_equal(read(), exp)


def test_host_array_depth_pitched(sva, engine):
    """sva_array_depth: copy_plane in multi.cpp."""
    W, H, D = 97, 33, 64
    imgs = list(synth.array_views(H, W, [(0, 0), (1, 0), (0, 1)], synth.array_delta(H, W, 9),
                                  seed=3))
    pairs = []
    for j in (1, 2):
        sx, sy, k = synth.pair_step((0, 0), [(0, 0), (1, 0), (0, 1)][j])
        pairs.append((0, j, sva.default_params(D=D, dir=sx, dir_y=sy), 0.05 * k))
    f, ps = 0.05, 0.036 / W
    want = engine.array_depth(imgs, pairs, [0, 2], f, ps, want_maps=True)
    hv = [host_view(a, 20 + i) for i, a in enumerate(imgs)]
    fr = sva._ArrayFrame(imgs, pairs, [0, 2])
    assert fr.head[2:5] == (W, H, W)            # (..., width, height, pitch, ...): pitch is head[4]
    head = (sva._ptr_table([v[1] for v in hv]),) + fr.head[1:4] + (hv[0][2],) + fr.head[5:]
    depth, nv, maps = fr.planes(1, np.float64), fr.planes(1, np.uint8), fr.planes(2, np.uint16)
    engine._chk(sva.lib.sva_array_depth(engine.h, *head, f, ps, depth.ctypes.data, nv.ctypes.data,
                                        maps.ctypes.data))
    for got, exp in zip((depth, nv, maps), want):
        assert np.array_equal(bits(got), bits(exp))
    assert (nv > 0).any() and len(np.unique(maps)) > 4
