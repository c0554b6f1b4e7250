"""sva_array_depth_rectified on the engine, on the banded
scene of tests/wmed_scene.py (128 x 96, D 32, nine groups) seen through a rig
that is not ideal: every view rolled, shifted and distorted in numpy, the model
that undoes it supplied as `rect`.

(a) SVA_ARRAY_GROUPS (check 1, sub 1) and SVA_ARRAY_PAIRS, mask 0 and 1: every
    plane equals the stand-alone composition -- sva_rectify, the route's plain job
    maps on the rectified views, sva_mask_maps, sva_cross_check,
    sva_filter_speckles, sva_fill_holes, sva_weighted_median, sva_fuse_depth_sub --
    byte for byte.
(b) identity rect, mask 0: sva_array_depth_smoothed's outputs; with wmed_radius 0,
    sva_array_depth_filled's.
(c) rectified, smoothed, rectified through one engine: each a fresh engine's.
(d) against the scene's truth, fewer wrong pixels than the same entry given the
    raw views with identity rect (the counts: profiles/rectify/README.md).
"""
import functools

import numpy as np
import pytest

import rectify_expect as re_
import wmed_expect as we
import wmed_scene as ws

pytestmark = pytest.mark.gpu

PAIRS, GROUPS = 0, 1
SPECKLE, FILL, R, SIGMA = (20, 1), (16, 3), 5, 32
ALL = dict(want_sub=True, want_maps=True, want_costs=True, want_size=True, want_found=True,
           want_support=True, want_views=True, want_valid=True)
# per view: roll in degrees, shift in pixels, k1 (focal length W pixels, centre of the image)
MODELS = [(0.8, (1.5, -2.0), -0.06), (-0.6, (-2.0, 1.25), 0.05), (0.5, (0.75, 2.5), -0.08),
          (-0.9, (2.25, 1.0), 0.04), (0.7, (-1.25, -1.75), -0.05), (-0.4, (1.0, 2.0), 0.07),
          (0.6, (-2.5, 0.5), -0.04), (-0.7, (0.5, -2.25), 0.06), (0.9, (2.0, -1.0), -0.07)]


def bilinear(img, x, y):
    """f64 bilinear sample with edge replication."""
    H, W = img.shape
    x = np.clip(x, 0, W - 1.0)
    y = np.clip(y, 0, H - 1.0)
    x0 = np.minimum(np.floor(x).astype(int), W - 2)
    y0 = np.minimum(np.floor(y).astype(int), H - 2)
    a, b = x - x0, y - y0
    f = img.astype(np.float64)
    return ((1 - a) * (1 - b) * f[y0, x0] + a * (1 - b) * f[y0, x0 + 1] +
            (1 - a) * b * f[y0 + 1, x0] + a * b * f[y0 + 1, x0 + 1])


@functools.lru_cache(maxsize=None)
def rig():
    """(raw views, rect models as dicts): raw view v holds, at the raw position
    the model sends a rectified pixel to, the ideal view's value there.  The
    model's inverse is found by fixed-point iteration (it is close to a shift)."""
    raws, models = [], []
    yy, xx = np.mgrid[0:ws.H, 0:ws.W].astype(np.float64)
    for img, (roll, shift, k1) in zip(ws.views(), MODELS):
        m = re_.rolled(ws.W, ws.H, roll_deg=roll, shift=shift, persp=(0, 0), k1=k1)
        h = m["h"]

        def forward(x, y):
            u = h[0] * x + h[1] * y + h[2]
            v = h[3] * x + h[4] * y + h[5]
            xn, yn = (u - m["cx"]) / m["fx"], (v - m["cy"]) / m["fy"]
            rad = 1 + k1 * (xn * xn + yn * yn)
            return xn * rad * m["fx"] + m["cx"], yn * rad * m["fy"] + m["cy"]

        x, y = xx.copy(), yy.copy()
        for _ in range(30):
            fx, fy = forward(x, y)
            x, y = x - (fx - xx), y - (fy - yy)
        raw = np.clip(np.rint(bilinear(img, x, y)), 0, 255).astype(np.uint8)
        raw.setflags(write=False)
        raws.append(raw)
        models.append(m)
    return raws, models


def rect_of(sva, models):
    return [sva.RectifyView.make(v["h"], v["cx"], v["cy"], v["fx"], v["fy"],
                                 [v[k] for k in ("k1", "k2", "p1", "p2", "k3")]) for v in models]


def identity(sva):
    return [sva.RectifyView.make() for _ in range(9)]


def same(a, b):
    return a is not None and b is not None and a.tobytes() == b.tobytes() and a.shape == b.shape


def engine(sva):
    return sva.Multi([0], streams=2, flags=sva.SVA_MULTI_GATHER_PEER)


def frame_of(sva, route):
    """(jobs, group_start): the scene's nine groups; on PAIRS two groups of pairs --
    camera 4 against its eight neighbours, camera 0 against its three."""
    jobs, gs = ws.jobs(sva)
    if route != PAIRS:
        return jobs, gs
    mine = jobs[gs[4]:gs[5]] + jobs[gs[0]:gs[1]]
    return mine, [0, gs[5] - gs[4], gs[5] - gs[4] + gs[1] - gs[0]]


def chain_kw(sva, route, radius=R):
    check = 1 if route == GROUPS else 0
    return dict(wmed_radius=radius, wmed_weights=we.weights(SIGMA), wmed_min_support=3,
                wmed_select=0, fill_max_dist=FILL[0], fill_min_found=FILL[1],
                fill_mode=sva.SVA_FILL_MEDIAN, speckle_max_size=SPECKLE[0],
                speckle_max_diff=SPECKLE[1], check=check, view_step=ws.VIEW_STEP if check else None,
                route=route, mode=sva.SVA_FUSE_MEDIAN, sub=1, **(ws.CHECK if check else {}))


def rectified(m, sva, route, views, rect, mask, border=0, radius=R, **want):
    jobs, gs = frame_of(sva, route)
    return m.array_depth_rectified(views, rect, jobs, gs, ws.F, ws.PS, border=border, mask=mask,
                                   **chain_kw(sva, route, radius), **want)


def assert_same(got, ref, which, skip=()):
    for k in ref:
        if k in skip:
            continue
        if ref[k] is None:
            assert got[k] is None, (which, k)
        else:
            assert same(got[k], ref[k]), (which, k)


@pytest.mark.parametrize("route,mask", [(GROUPS, 1), (GROUPS, 0), (PAIRS, 1), (PAIRS, 0)])
def test_frame_is_the_stand_alone_composition(sva, ctx, route, mask):
    raws, models = rig()
    rect = rect_of(sva, models)
    jobs, gs = frame_of(sva, route)
    n_groups = len(gs) - 1
    want = dict(ALL, want_counts=route == GROUPS, want_n_valid=route == PAIRS)
    m = engine(sva)
    try:
        new = rectified(m, sva, route, raws, rect, mask, border=9, **want)
        bare = rectified(m, sva, route, raws, rect, mask, border=9)
        # 1. sva_rectify
        views, valid, _ = ctx.rectify(np.stack(raws), rect, border=9, want_valid=True)
        # 2. the route's plain job maps on the rectified views
        _, _, _, sub, maps, cmin, csec = m.array_depth_sub(
            list(views), jobs, gs, ws.F, ws.PS, route=route, mode=sva.SVA_FUSE_MEDIAN,
            want_sub=True, want_maps=True, want_costs=True)
    finally:
        m.close()
    used = sorted({j[0] for j in jobs} | {j[1] for j in jobs})
    assert same(new["views"][used], views[used]) and same(new["valid"][used], valid[used])
    unused = [v for v in range(9) if v not in used]
    assert not new["views"][unused].any() and not new["valid"][unused].any()
    eo, ev, _ = re_.rectify(np.stack(raws), models, border=9)
    assert np.array_equal(views, eo) and np.array_equal(valid, ev) and 0.8 < valid.mean() < 1.0
    # 3. the chain
    refs = [jobs[j][0] for j in (range(len(jobs)) if route == PAIRS else gs[:-1])]
    d, s = maps, sub
    if mask:
        d, s = ctx.mask_maps(d, valid[refs], ws.INVALID, s)
        assert (d != maps).sum() > 100
    agree = conflict = None
    if route == GROUPS:
        d, s, agree, conflict = ctx.cross_check(d, ws.VIEW_STEP, s, ws.INVALID, **ws.CHECK)
    d, s, size = ctx.filter_speckles(d, SPECKLE[0], SPECKLE[1], s, ws.INVALID)
    d, s, found = ctx.fill_holes(d, FILL[0], FILL[1], sva.SVA_FILL_MEDIAN, s, ws.INVALID)
    d, s, support = ctx.weighted_median(d, R, list(views[refs]), we.weights(SIGMA), s, None, 3, 1,
                                        ws.INVALID)
    for name, plane in (("maps", d), ("subpix", s), ("comp_size", size), ("n_found", found),
                        ("support", support), ("cost_min", cmin), ("cost_second", csec)):
        assert same(new[name], plane), name
    if route == GROUPS:
        assert same(new["agree"], agree) and same(new["conflict"], conflict)
    # 4. the fusion
    for k in range(n_groups):
        sl = slice(gs[k], gs[k + 1]) if route == PAIRS else slice(k, k + 1)
        bases = [j[3] for j in jobs[gs[k]:gs[k + 1]]] if route == PAIRS else [ws.PITCH_M]
        depth, nv = ctx.fuse_depth_sub(d[sl], s[sl], bases, ws.F, ws.PS)
        assert same(new["depth"][k], depth.reshape(ws.H, ws.W)), k
        if route == PAIRS:
            assert same(new["n_valid"][k], nv.reshape(ws.H, ws.W)), k
    assert same(bare["depth"], new["depth"])
    assert all(bare[k] is None for k in bare if k != "depth")


@pytest.mark.parametrize("route", [GROUPS, PAIRS])
def test_identity_rect_is_the_smoothed_and_the_filled_entry(sva, route):
    jobs, gs = frame_of(sva, route)
    want = {k: v for k, v in ALL.items() if k not in ("want_views", "want_valid")}
    want.update(want_counts=route == GROUPS, want_n_valid=route == PAIRS)
    kw = chain_kw(sva, route)
    m = engine(sva)
    try:
        new = rectified(m, sva, route, ws.views(), identity(sva), 0, want_views=True,
                        want_valid=True, **want)
        old = m.array_depth_smoothed(ws.views(), jobs, gs, ws.F, ws.PS, **kw, **want)
        off = rectified(m, sva, route, ws.views(), identity(sva), 0, radius=0, **want)
        kw0 = {k: v for k, v in kw.items() if not k.startswith("wmed_")}
        filled = m.array_depth_filled(ws.views(), jobs, gs, ws.F, ws.PS, **kw0,
                                      **{k: v for k, v in want.items() if k != "want_support"})
    finally:
        m.close()
    assert_same(new, old, "smoothed")
    assert_same(off, filled, "filled")
    assert not off["support"].any() and old["support"].any()
    used = sorted({j[0] for j in jobs} | {j[1] for j in jobs})
    assert same(new["views"][used], np.stack(ws.views())[used]) and new["valid"][used].all()
    assert not same(new["maps"], off["maps"])


def test_three_frames_through_one_engine(sva):
    raws, models = rig()

    def rect_frame(m):
        return rectified(m, sva, GROUPS, raws, rect_of(sva, models), 1, **dict(ALL, want_counts=True))

    def smooth_frame(m):
        jobs, gs = frame_of(sva, PAIRS)
        return m.array_depth_smoothed(ws.views(), jobs, gs, ws.F, ws.PS, **chain_kw(sva, PAIRS),
                                      want_maps=True, want_sub=True, want_support=True)

    def alone(frame):
        m = sva.Multi([0])
        try:
            return frame(m)
        finally:
            m.close()

    ref_rect, ref_smooth = alone(rect_frame), alone(smooth_frame)
    m = sva.Multi([0])
    try:
        first, second, third = rect_frame(m), smooth_frame(m), rect_frame(m)
    finally:
        m.close()
    assert ref_rect["maps"].any() and ref_rect["valid"].any() and ref_smooth["maps"].any()
    assert_same(first, ref_rect, "first")
    assert_same(second, ref_smooth, "second")
    assert_same(third, ref_rect, "third")


def test_rectifying_leaves_fewer_wrong_pixels(sva):
    """The same entry on the same raw views, with the rig's models and with
    identity: the direction only."""
    raws, models = rig()
    m = engine(sva)
    try:
        good = rectified(m, sva, GROUPS, raws, rect_of(sva, models), 1, want_maps=True)
        bad = rectified(m, sva, GROUPS, raws, identity(sva), 1, want_maps=True)
    finally:
        m.close()
    q_good, q_bad = ws.quality(good["maps"]), ws.quality(bad["maps"])
    print("wrong, correct, holes: rectified %s, raw %s" % (q_good, q_bad))
    assert q_good[0] < q_bad[0]
    assert q_good[1] > q_bad[1]


def test_refusals_write_nothing(sva):
    """The entry's own refusals come after the smoothed entry's, in order; nothing
    is launched and the canary-filled outputs stay."""
    INV = sva.SVA_ERR_INVALID_ARG
    counted = ("rectify", "mask_maps", "census", "cost", "sgm_paths", "wta_hv", "wmed", "fuse_depth")
    nan = float("nan")
    ok = identity(sva)

    def broken(i, **ch):
        r = identity(sva)
        r[i] = sva.RectifyView.make(**ch)
        return r

    cases = [
        ("null_rect", "null rect", dict(rect=None, border=300)),
        ("view_h", "non-finite entry (view 3)", dict(rect=broken(3, h=(nan,) * 9), border=300)),
        ("view_f", "fx, fy must be finite and > 0 (view 8)", dict(rect=broken(8, fy=0.0), mask=2)),
        ("border", "border must be 0..255", dict(border=256, mask=2)),
        ("mask", "mask must be 0 or 1", dict(mask=-1)),
        # the old rules first, a radius of 0 allowed
        ("radius_16", "wmed radius must be 1..15", dict(r=16, rect=None)),
        ("select", "wmed select must be 0 or 1", dict(r=0, sel=2, rect=None)),
        ("fill_mode", "fill mode must be 0..2", dict(fm=3, rect=None)),
    ]
    w = we.weights(SIGMA)
    jobs, gs = frame_of(sva, GROUPS)
    m = engine(sva)
    try:
        c0 = m.context(0, 0)
        c0.set_timing(sva.SVA_TIMING_ALL)
        c0.reset_timing()
        fr = sva._ArrayFrame(ws.views(), jobs, gs)
        for name, text, ch in cases:
            a = dict(fm=2, r=R, sel=0, rect=ok, border=0, mask=1)
            a.update(ch)
            depth = np.full((fr.G, ws.H, ws.W), -7.0, np.float64)
            maps = np.full((fr.G, ws.H, ws.W), 0x5A5A, np.uint16)
            views = np.full((9, ws.H, ws.W), 0x6B, np.uint8)
            valid = np.full((9, ws.H, ws.W), 0x6B, np.uint8)
            st = sva.lib.sva_array_depth_rectified(
                m.h, *fr.head, GROUPS, None, ws.F, ws.PS, 0, sva.SVA_FUSE_MEDIAN,
                depth.ctypes.data, None, None, None, maps.ctypes.data, None, None, None, 0, 1, 2, 8,
                None, None, 0, 20, 1, None, 16, 3, a["fm"], None, a["r"], w.ctypes.data, 1, a["sel"],
                None, sva._view_table(a["rect"]), a["border"], a["mask"], views.ctypes.data,
                valid.ctypes.data)
            msg = sva.lib.sva_multi_last_error(m.h).decode()
            assert st == INV and text in msg, (name, st, msg)
            assert (depth == -7.0).all() and (maps == 0x5A5A).all()
            assert (views == 0x6B).all() and (valid == 0x6B).all()
        assert {k: c0.kernel_time(k)[1] for k in counted} == dict.fromkeys(counted, 0)
        # the engine still works: one rectify launch for the nine views, one mask per job
        rectified(m, sva, GROUPS, ws.views(), ok, 1)
        assert c0.kernel_time("rectify")[1] == 1 and c0.kernel_time("mask_maps")[1] == 9
    finally:
        m.close()


def test_across_devices(sva):
    n = min(sva.device_count(), 4)
    if n < 2:
        pytest.skip("needs >= 2 HIP devices")
    raws, models = rig()
    def frames(m):
        return {r: rectified(m, sva, r, raws, rect_of(sva, models), 1,
                             **dict(ALL, want_n_valid=r == PAIRS, want_counts=r == GROUPS))
                for r in (GROUPS, PAIRS)}

    one = engine(sva)
    try:
        ref = frames(one)
    finally:
        one.close()
    for flags in (sva.SVA_MULTI_GATHER_RCCL, sva.SVA_MULTI_GATHER_PEER):
        m = sva.Multi(list(range(n)), streams=2, flags=flags)
        try:
            got = frames(m)
        finally:
            m.close()
        for r in got:
            assert_same(got[r], ref[r], (r, flags))
