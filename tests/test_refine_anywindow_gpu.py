"""improveWithDisparity at any window on the GPU vs the CPU oracle: the box-sum
route of refine.hip (summed-area tables of the 11 absolute-difference planes,
DESIGN.md §2.7 / §4.2), which takes every k = (window-1)/2 >= 17 and, forced
through SVA_DEBUG_REFINE_ROUTE, the small k where refine_box_kernel is an
independent witness.

Every comparison is byte-exact against oracle.improve_with_disparity on a
random `init`, so pixels that must stay unwritten are checked too.  Inputs as
in tests/test_refine_gpu.py: synth.texture, synth.reference_array(0.036 / W),
rng.integers(0, 40) disparities.  Pairs (12,11), (12,7), (12,6) step along
(ddx, ddy) = (1,0), (0,1), (1,1); (12,13) and (12,17) give (0,0): their 11
windows coincide, so they only test the first-minimum rule."""
import functools

import numpy as np
import pytest
import torch

from stereovisionarray_amd import synth

pytestmark = pytest.mark.gpu

ROUTE_BOX, ROUTE_DIRECT, ROUTE_SAT = 0, 1, 2
DIRS = {11: (1, 0), 7: (0, 1), 6: (1, 1), 13: (0, 0), 17: (0, 0)}
FIVE = (11, 13, 7, 17, 6)


def cam_pair(sva, oracle, b, W):
    cams = synth.reference_array(0.036 / W)
    return ((sva.Camera.make(*cams[12]), sva.Camera.make(*cams[b])),
            (oracle.OCamera.make(*cams[12]), oracle.OCamera.make(*cams[b])))


@functools.lru_cache(maxsize=None)
def recipe(W, H, window, masked):
    """Planes of one case; the paired image of camera b is texture(100 + its
    index in FIVE).  Read-only."""
    rng = np.random.default_rng(window)
    center = synth.texture(H, W, window)
    imgs = {b: synth.texture(H, W, 100 + i) for i, b in enumerate(FIVE)}
    disp = rng.integers(0, 40, size=(H, W)).astype(np.uint8)
    mask = (rng.random((H, W)) < 0.7).astype(np.uint8) if masked else None
    init = rng.integers(0, 256, size=(H, W)).astype(np.uint8)
    for a in (center, disp, init, *imgs.values()) + ((mask,) if masked else ()):
        a.setflags(write=False)
    return center, imgs, disp, mask, init


_expected = {}


def expected(oracle, sva, W, H, window, masked, bs):
    """Oracle output of one case for the pair list bs, computed once."""
    key = (W, H, window, masked, bs)
    if key not in _expected:
        center, imgs, disp, mask, init = recipe(W, H, window, masked)
        st, exp = oracle.improve_with_disparity(
            disp, center, [imgs[b] for b in bs], [cam_pair(sva, oracle, b, W)[1] for b in bs],
            window=window, mask=mask, init=init)
        assert st == 0
        exp.setflags(write=False)
        _expected[key] = exp
    return _expected[key]


def winners(exp, disp, mask, W, H, window, b):
    """Candidates that win somewhere on the pixels pair b writes."""
    k = (window - 1) // 2
    ddx, ddy = DIRS[b]
    wr = np.zeros((H, W), bool)
    wr[k + 5 * ddy:H - k - 5 * ddy + 1, k + 5 * ddx:W - k - 5 * ddx + 1] = True
    if mask is not None:
        wr &= mask != 0
    c = (exp[wr].astype(np.int64) - disp[wr] + 128) % 256 - 128
    assert (c % (ddx + ddy) == 0).all()
    return set((c // (ddx + ddy) + 5).tolist())


CASES = [(150, 110, 67, True), (150, 110, 68, True), (150, 124, 81, True), (190, 170, 129, False)]


@pytest.mark.parametrize("bs", [(11,), (7,), (6,), (13,), FIVE], ids=lambda bs: "-".join(map(str, bs)))
@pytest.mark.parametrize("W,H,window,masked", CASES)
def test_windows_past_old_cap(ctx, sva, oracle, W, H, window, masked, bs):
    center, imgs, disp, mask, init = recipe(W, H, window, masked)
    exp = expected(oracle, sva, W, H, window, masked, bs)
    if len(bs) == 1 and sum(DIRS[bs[0]]):
        won = winners(exp, disp, mask, W, H, window, bs[0])
        assert len(won) >= 5, won           # the sums decide, not one lucky candidate
    assert (exp != init).any() and (exp == init).any()
    got = ctx.improve_with_disparity(disp, center, [imgs[b] for b in bs],
                                     [cam_pair(sva, oracle, b, W)[0] for b in bs], window=window,
                                     mask=mask, init=init)
    assert ctx.get_debug(sva.SVA_DEBUG_REFINE_LAST_ROUTE) == ROUTE_SAT
    assert np.array_equal(got, exp)


def test_every_candidate_wins_somewhere(sva, oracle):
    """Coverage of the module's expected planes: over the positive directions
    of the cases above, each of the 11 candidates is some pixel's answer."""
    seen = set()
    for W, H, window, masked in CASES:
        _, _, disp, mask, _ = recipe(W, H, window, masked)
        for b in (11, 7, 6):
            seen |= winners(expected(oracle, sva, W, H, window, masked, (b,)), disp, mask, W, H,
                            window, b)
    assert seen == set(range(11))


@pytest.mark.parametrize("b", [11, 7, 6, 13])
def test_first_minimum_on_ties(ctx, sva, oracle, b):
    """Constant planes: all 11 SADs are equal, candidate 0 wins,
    out = (uchar)(d - 5 (ddx + ddy))."""
    W, H, window = 150, 110, 67
    k = 33
    ddx, ddy = DIRS[b]
    rng = np.random.default_rng(b)
    center = np.full((H, W), 77, np.uint8)
    img = np.zeros((H, W), np.uint8)          # the shifted plane is 0 wherever it is not image
    disp = rng.integers(0, 40, size=(H, W)).astype(np.uint8)
    init = rng.integers(0, 256, size=(H, W)).astype(np.uint8)
    pair, opair = cam_pair(sva, oracle, b, W)
    st, exp = oracle.improve_with_disparity(disp, center, [img], [opair], window=window, init=init)
    ys, xs = slice(k + 5 * ddy, H - k - 5 * ddy + 1), slice(k + 5 * ddx, W - k - 5 * ddx + 1)
    want = init.copy()
    want[ys, xs] = (disp[ys, xs].astype(np.int64) - 5 * (ddx + ddy)).astype(np.uint8)
    assert st == 0 and np.array_equal(exp, want)
    got = ctx.improve_with_disparity(disp, center, [img], [pair], window=window, init=init)
    assert ctx.get_debug(sva.SVA_DEBUG_REFINE_LAST_ROUTE) == ROUTE_SAT
    assert np.array_equal(got, exp)


# Edges of the route's work split: the row pass scans 1024 columns per round,
# the column pass walks 8 rows per step and the bounding-box pass 16, the pick
# pass tiles 64 x 4 pixels.  (1100, 70): two scan rounds, the second partial;
# (90, 301): 37 full column steps and a remainder of 5; (76, 76) with the
# diagonal pair: exactly one pixel passes the window test; (75, 76) / (76, 75):
# none does.
@pytest.mark.parametrize("W,H,bs,masked", [
    (1100, 70, (11,), False), (1100, 70, (13, 11), True), (90, 301, (7,), False),
    (90, 301, (6, 7), True), (76, 76, (6,), False), (75, 76, (6,), False), (76, 75, (6,), False),
    (1091, 67, (11,), False)])
def test_chunk_and_strip_edges(ctx, sva, oracle, W, H, bs, masked):
    window = 67
    center, imgs, disp, mask, init = recipe(W, H, window, masked)
    exp = expected(oracle, sva, W, H, window, masked, bs)
    n_written = int((exp != init).sum())
    if (W, H) == (76, 76):
        assert np.argwhere(exp != init).tolist() in ([[38, 38]], [])
    if 75 in (W, H):
        assert n_written == 0
    got = ctx.improve_with_disparity(disp, center, [imgs[b] for b in bs],
                                     [cam_pair(sva, oracle, b, W)[0] for b in bs], window=window,
                                     mask=mask, init=init)
    assert ctx.get_debug(sva.SVA_DEBUG_REFINE_LAST_ROUTE) == ROUTE_SAT
    assert np.array_equal(got, exp)


def test_single_pixel_is_written(ctx, sva, oracle):
    """W = 2k + 10 ddx, H = 2k + 10 ddy: the one pixel that passes the window
    test gets its value (an `init` chosen so that the write is visible)."""
    W = H = 76
    center, imgs, disp, _, _ = recipe(W, H, 67, False)
    pair, opair = cam_pair(sva, oracle, 6, W)
    exps = []
    for fill in (0, 255):
        init = np.full((H, W), fill, np.uint8)
        st, exp = oracle.improve_with_disparity(disp, center, [imgs[6]], [opair], window=67,
                                                init=init)
        got = ctx.improve_with_disparity(disp, center, [imgs[6]], [pair], window=67, init=init)
        assert st == 0 and np.array_equal(got, exp)
        assert np.argwhere(exp != fill).tolist() in ([[38, 38]], [])
        exps.append(exp)
    # a written pixel does not depend on init: the same value over both fills
    assert exps[0][38, 38] == exps[1][38, 38]


@pytest.mark.parametrize("W,H,window", [(301, 150, 67), (301, 150, 69), (140, 203, 129)])
def test_padded_pitch_sparse_mask(ctx, sva, oracle, torch_dev, W, H, window):
    """Device entry point on planes with pitch = W + 13 and random bytes in
    the padding, a 2 % mask (so the bounding box is ragged), the four steps.
    The output padding stays untouched."""
    P = W + 13
    rng = np.random.default_rng(W * 1000 + window)
    center = synth.texture(H, W, 3)
    pairs, opairs, imgs = [], [], []
    for i, b in enumerate((13, 7, 11, 6)):
        p, o = cam_pair(sva, oracle, b, W)
        pairs.append(p); opairs.append(o)
        imgs.append(synth.texture(H, W, 60 + i))
    disp = rng.integers(0, 12, size=(H, W)).astype(np.uint8)
    mask = (rng.random((H, W)) < 0.02).astype(np.uint8)
    init = rng.integers(0, 256, size=(H, W)).astype(np.uint8)

    def padded(a):
        full = rng.integers(0, 256, size=(H, P)).astype(np.uint8)
        full[:, :W] = a
        return torch.from_numpy(full).to(torch_dev)

    dd, dc, dm = padded(disp), padded(center), padded(mask)
    di = [padded(im) for im in imgs]
    out = padded(init)
    pad_before = out[:, W:].cpu().numpy().copy()
    ctx.improve_with_disparity_d(dd.data_ptr(), dc.data_ptr(), [t.data_ptr() for t in di], pairs,
                                 W, H, P, dm.data_ptr(), window, False, out.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    assert ctx.get_debug(sva.SVA_DEBUG_REFINE_LAST_ROUTE) == ROUTE_SAT
    st, exp = oracle.improve_with_disparity(disp, center, imgs, opairs, window=window, mask=mask,
                                            init=init)
    got = out.cpu().numpy()
    assert st == 0 and (exp != init).any()
    assert np.array_equal(got[:, :W], exp)
    assert np.array_equal(got[:, W:], pad_before)


@pytest.mark.parametrize("window,auto_route", [(3, ROUTE_BOX), (4, ROUTE_BOX), (21, ROUTE_BOX),
                                               (33, ROUTE_BOX), (35, ROUTE_SAT),
                                               (65, ROUTE_SAT)])
def test_forced_route_at_small_windows(ctx, sva, oracle, window, auto_route):
    """The box-sum route forced at small windows, on the (150, 110) frame of
    test_improve_with_disparity_windows: equal to the oracle and to the
    automatic route byte for byte.  Up to window 33 (k = 16) the automatic route
    is refine_box_kernel, an independent witness; from 35 it is the box-sum
    route itself (the measured default)."""
    W, H = 150, 110
    center, imgs, disp, mask, init = recipe(W, H, window, True)
    exp = expected(oracle, sva, W, H, window, True, FIVE)
    pairs = [cam_pair(sva, oracle, b, W)[0] for b in FIVE]
    il = [imgs[b] for b in FIVE]
    assert ctx.get_debug(sva.SVA_DEBUG_REFINE_ROUTE) == 0
    auto = ctx.improve_with_disparity(disp, center, il, pairs, window=window, mask=mask, init=init)
    assert ctx.get_debug(sva.SVA_DEBUG_REFINE_LAST_ROUTE) == auto_route
    ctx.set_debug(sva.SVA_DEBUG_REFINE_ROUTE, 1)
    try:
        assert ctx.get_debug(sva.SVA_DEBUG_REFINE_ROUTE) == 1
        forced = ctx.improve_with_disparity(disp, center, il, pairs, window=window, mask=mask,
                                            init=init)
        assert ctx.get_debug(sva.SVA_DEBUG_REFINE_LAST_ROUTE) == ROUTE_SAT
    finally:
        ctx.set_debug(sva.SVA_DEBUG_REFINE_ROUTE, 0)
    assert ctx.get_debug(sva.SVA_DEBUG_REFINE_ROUTE) == 0
    assert np.array_equal(forced, exp)
    assert np.array_equal(forced, auto)


def test_route_key_limits(ctx, sva):
    for bad in (-1, 2):
        with pytest.raises(sva.SvaError) as e:
            ctx.set_debug(sva.SVA_DEBUG_REFINE_ROUTE, bad)
        assert e.value.status == sva.SVA_ERR_INVALID_ARG
    with pytest.raises(sva.SvaError) as e:
        ctx.set_debug(sva.SVA_DEBUG_REFINE_LAST_ROUTE, 0)      # read-only
    assert e.value.status == sva.SVA_ERR_INVALID_ARG
    for op in (lambda: ctx.set_debug(99, 0), lambda: ctx.get_debug(99)):
        with pytest.raises(sva.SvaError) as e:
            op()
        assert e.value.status == sva.SVA_ERR_INVALID_ARG
    assert ctx.get_debug(sva.SVA_DEBUG_REFINE_ROUTE) == 0
    # window 1 (k = 0) stays on refine_kernel<0> even when the route is forced
    ctx.set_debug(sva.SVA_DEBUG_REFINE_ROUTE, 1)
    try:
        z = np.zeros((8, 8), np.uint8)
        cams = synth.reference_array(0.036 / 8)
        ctx.improve_with_disparity(z, z, [z], [(sva.Camera.make(*cams[12]),
                                                sva.Camera.make(*cams[11]))], window=1)
        assert ctx.get_debug(sva.SVA_DEBUG_REFINE_LAST_ROUTE) == ROUTE_DIRECT
    finally:
        ctx.set_debug(sva.SVA_DEBUG_REFINE_ROUTE, 0)


def test_strict_and_impossible_windows(ctx, sva, oracle):
    W, H = 150, 110
    center, imgs, disp, _, init = recipe(W, H, 67, True)
    pair, opair = cam_pair(sva, oracle, 11, W)
    run = functools.partial(ctx.improve_with_disparity, disp, center, [imgs[11]], [pair])
    orun = functools.partial(oracle.improve_with_disparity, disp, center, [imgs[11]], [opair])
    # window 67, strict: a full mask has border pixels whose windows leave the image
    for mask in (None, np.ones((H, W), np.uint8)):
        with pytest.raises(sva.SvaError) as e:
            run(window=67, strict=True, mask=mask, init=init)
        assert e.value.status == sva.SVA_ERR_INVALID_ARG
        assert orun(window=67, strict=True, mask=mask, init=init)[0] == -1
    # a mask inside the valid region [38, 112] x [33, 77] succeeds, edges included
    inside = np.zeros((H, W), np.uint8)
    inside[33:78, 38:113] = 1
    st, exp = orun(window=67, strict=True, mask=inside, init=init)
    assert st == 0 and (exp[inside == 1] != init[inside == 1]).any()
    assert np.array_equal(run(window=67, strict=True, mask=inside, init=init), exp)
    one_out = inside.copy()
    one_out[33, 37] = 1                       # one pixel left of the region
    with pytest.raises(sva.SvaError) as e:
        run(window=67, strict=True, mask=one_out, init=init)
    assert e.value.status == sva.SVA_ERR_INVALID_ARG
    # a window no image position can hold: nothing is written, only the mask
    # decides the fault
    for window in (2 * W + 1, 2 ** 31 - 1):
        got = run(window=window, init=init)
        assert ctx.get_debug(sva.SVA_DEBUG_REFINE_LAST_ROUTE) == ROUTE_SAT
        assert np.array_equal(got, init)
        assert np.array_equal(run(window=window, mask=inside, init=init), init)
        for mask in (None, inside):
            with pytest.raises(sva.SvaError) as e:
                run(window=window, strict=True, mask=mask, init=init)
            assert e.value.status == sva.SVA_ERR_INVALID_ARG
        empty = np.zeros((H, W), np.uint8)
        assert np.array_equal(run(window=window, strict=True, mask=empty, init=init), init)
    st, exp = orun(window=2 * W + 1, init=init)
    assert st == 0 and np.array_equal(exp, init)
    for window in (0, -5):
        with pytest.raises(sva.SvaError) as e:
            run(window=window, init=init)
        assert e.value.status == sva.SVA_ERR_UNSUPPORTED


def test_sums_past_32_bits(ctx, sva, oracle):
    """k = 2053 is the first k whose window SAD can reach 2^32.  centre = 0,
    disparity = 1 and a unit step in x make shifted(x) = image(x + 1); the
    image is 255 except columns 0..10.  At the three masked pixels candidate 0
    has the smallest SAD (its window holds the most zero columns), at least one
    SAD is >= 2^32, and sums kept modulo 2^32 would choose another candidate."""
    W, H, window, k = 4120, 4110, 4107, 2053
    center = np.zeros((H, W), np.uint8)
    disp = np.ones((H, W), np.uint8)
    img = np.full((H, W), 255, np.uint8)
    img[:, :11] = 0
    pts = [(2058, 2053), (2060, 2055), (2062, 2057)]
    mask = np.zeros((H, W), np.uint8)
    for x, y in pts:
        mask[y, x] = 1
    init = np.random.default_rng(8).integers(0, 256, size=(H, W)).astype(np.uint8)
    shifted_row = np.zeros(W, np.int64)
    shifted_row[:W - 1] = img[0, 1:]
    for x, _ in pts:
        sad = np.array([2 * k * shifted_row[x - k + c - 5:x + k + c - 5].sum() for c in range(11)],
                       np.int64)
        assert sad.max() >= 2 ** 32
        assert int(np.argmin(sad)) == 0
        assert int(np.argmin(sad % 2 ** 32)) != 0
    c0 = sva.Camera.make(0.05, (1.0, 0.0, 0.0), 1e-4)
    c1 = sva.Camera.make(0.05, (0.0, 0.0, 0.0), 1e-4)
    o0 = oracle.OCamera.make(0.05, (1.0, 0.0, 0.0), 1e-4)
    o1 = oracle.OCamera.make(0.05, (0.0, 0.0, 0.0), 1e-4)
    st, exp = oracle.improve_with_disparity(disp, center, [img], [(o0, o1)], window=window,
                                            mask=mask, strict=True, init=init)
    assert st == 0
    for x, y in pts:
        assert exp[y, x] == 252
    got = ctx.improve_with_disparity(disp, center, [img], [(c0, c1)], window=window, mask=mask,
                                     strict=True, init=init)
    assert ctx.get_debug(sva.SVA_DEBUG_REFINE_LAST_ROUTE) == ROUTE_SAT
    assert np.array_equal(got, exp)
