"""sva_array_depth_smoothed on the engine, on the banded
scene of tests/wmed_scene.py, through the three routes with sub 0 / 1 and
wmed_select 0 / 1.  Bit for bit: the maps, f32 maps, n_found and support are
tests/wmed_expect.py's of tests/fill_expect.py's of the filled frame's inputs --
on the group route from the CPU oracle's maps through cross_expect,
speckle_expect, fill_expect and wmed_expect, with no GPU plane in the chain --
depth is the matching sva_fuse_depth* of them; wmed_select 1 with fill_max_dist 0
is sva_array_depth_filled; the new refusals come after the old ones."""
import numpy as np
import pytest

import fill_expect as fe
import speckle_expect as se
import wmed_expect as we
import wmed_scene as ws

pytestmark = pytest.mark.gpu

PAIRS, GROUPS, MIXED = 0, 1, 2
UNIT = [ws.PITCH_M] * 9
SPECKLE = (20, 1)
FILL = (16, 3)
R, SIGMA = 5, 32
ALL = dict(want_sub=True, want_maps=True, want_costs=True, want_size=True, want_found=True,
           want_support=True)


def same(a, b):
    return a is not None and b is not None and a.tobytes() == b.tobytes() and a.shape == b.shape


def engine(sva):
    return sva.Multi([0], streams=2, flags=sva.SVA_MULTI_GATHER_PEER)


def frame_of(sva, route):
    """(jobs, group_start, unit): the scene's groups; on PAIRS two center-style
    groups -- camera 4 against its eight neighbours, camera 0 against its three."""
    if route != PAIRS:
        jobs, gs = ws.jobs(sva, route == MIXED)
        return jobs, gs, UNIT if route == MIXED else None
    jobs, gs = ws.jobs(sva)
    mine = jobs[gs[4]:gs[5]] + jobs[gs[0]:gs[1]]
    return mine, [0, gs[5] - gs[4], gs[5] - gs[4] + gs[1] - gs[0]], None


def frame_args(sva, route, check, sub):
    jobs, gs, unit = frame_of(sva, route)
    return (ws.views(), jobs, gs, ws.F, ws.PS), dict(
        check=check, view_step=ws.VIEW_STEP if check else None, route=route, unit_baseline=unit,
        mode=sva.SVA_FUSE_MEDIAN, sub=sub, speckle_max_size=SPECKLE[0],
        speckle_max_diff=SPECKLE[1], **(ws.CHECK if check else {}))


def smoothed(m, sva, route, check, sub, select, fill=FILL, guided=True, ms=1, **want):
    pos, kw = frame_args(sva, route, check, sub)
    return m.array_depth_smoothed(*pos, R, we.weights(SIGMA) if guided else None, ms, select,
                                  fill_max_dist=fill[0], fill_min_found=fill[1],
                                  fill_mode=sva.SVA_FILL_MEDIAN, **kw, **want)


def filled(m, sva, route, check, sub, fill=FILL, **want):
    pos, kw = frame_args(sva, route, check, sub)
    return m.array_depth_filled(*pos, fill[0], fill[1], sva.SVA_FILL_MEDIAN, **kw, **want)


def guides_of(sva, route):
    jobs, gs, _ = frame_of(sva, route)
    firsts = range(len(jobs)) if route == PAIRS else gs[:-1]
    return np.stack([ws.views()[jobs[j][0]] for j in firsts])


def expect_from(maps, subpix, n_found, guides, select, guided=True, ms=1):
    sel = n_found if select == 1 else None
    return we.weighted_median(maps, ws.INVALID, R, guides if guided else None,
                              we.weights(SIGMA) if guided else None, subpix, sel, ms, 1)


@pytest.mark.parametrize("sub", [0, 1])
@pytest.mark.parametrize("select", [0, 1])
def test_groups_against_the_cpu_chain(sva, ctx, select, sub):
    """SVA_ARRAY_GROUPS, check 1: every plane from the oracle's maps through the
    four CPU expectations."""
    d, s = ws.checked(**ws.CHECK)[:2]
    d, s, _ = se.filter_speckles(d, ws.INVALID, SPECKLE[0], SPECKLE[1], s)[:3]
    d, s, found, _ = fe.fill_holes(d, ws.INVALID, FILL[0], FILL[1], fe.MEDIAN, s)
    eo, es, en, written = expect_from(d, s, found, np.stack(ws.views()), select)
    m = engine(sva)
    try:
        new = smoothed(m, sva, GROUPS, 1, sub, select, want_counts=True,
                       **dict(ALL, want_sub=bool(sub)))
        bare = smoothed(m, sva, GROUPS, 1, sub, select)
    finally:
        m.close()
    assert np.array_equal(new["maps"], eo), int((new["maps"] != eo).sum())
    assert np.array_equal(new["support"], en) and np.array_equal(new["n_found"], found)
    assert written.sum() > 1000 and (eo != d).sum() > 100
    if select:
        assert np.array_equal(new["maps"][found == 0], d[found == 0])
    if sub:
        # the oracle's f32 planes agree with the engine's to 1e-5, not bit for bit:
        # the source pixels must be the same, so compare through the engine's own
        ok = we.valid(eo, ws.INVALID)
        assert np.allclose(new["subpix"][ok], es[ok], atol=1e-4)
    else:
        assert new["subpix"] is None
    for g in range(9):
        if sub:
            depth = ctx.fuse_depth_sub(new["maps"][g][None], new["subpix"][g][None], [ws.PITCH_M],
                                       ws.F, ws.PS)[0]
        else:
            depth = ctx.fuse_depth(new["maps"][g][None], [ws.PITCH_M], ws.F, ws.PS)[0]
        assert same(new["depth"][g], depth.reshape(ws.H, ws.W)), g
    assert same(bare["depth"], new["depth"])
    assert all(bare[k] is None for k in bare if k != "depth")


@pytest.mark.parametrize("route,check,sub,select,guided", [
    (MIXED, 0, 1, 0, True), (MIXED, 0, 0, 1, False), (PAIRS, 0, 1, 1, True),
    (PAIRS, 0, 0, 0, True), (GROUPS, 1, 1, 0, False)])
def test_routes_against_the_filled_frame(sva, ctx, route, check, sub, select, guided):
    """Every route: the smoothed frame is wmed_expect (and sva_weighted_median) of
    the filled frame's planes, bit for bit, the f32 planes included; depth is the
    fusion of the smoothed maps; the other planes are the filled frame's."""
    jobs, gs, _ = frame_of(sva, route)
    want = dict(ALL, want_sub=bool(sub), want_n_valid=route == PAIRS, want_counts=bool(check))
    m = engine(sva)
    try:
        new = smoothed(m, sva, route, check, sub, select, guided=guided, ms=3, **want)
        old = filled(m, sva, route, check, sub, **{k: v for k, v in want.items()
                                                   if k != "want_support"})
    finally:
        m.close()
    g = guides_of(sva, route)
    eo, es, en, written = expect_from(old["maps"], old["subpix"], old["n_found"], g, select,
                                      guided, 3)
    assert np.array_equal(new["maps"], eo) and np.array_equal(new["support"], en)
    assert written.sum() > 1000 and not np.array_equal(eo, old["maps"])
    if sub:
        assert same(new["subpix"], es)
    alone = ctx.weighted_median(old["maps"], R, list(g) if guided else None,
                                we.weights(SIGMA) if guided else None, old["subpix"],
                                old["n_found"] if select else None, 3, 1)
    assert same(new["maps"], alone[0]) and same(new["support"], alone[2])
    for name in ("cost_min", "cost_second", "comp_size", "n_found", "agree", "conflict"):
        assert (old[name] is None and new[name] is None) or same(new[name], old[name]), name
    n_groups = len(gs) - 1
    for k in range(n_groups):
        sl = slice(gs[k], gs[k + 1]) if route == PAIRS else slice(k, k + 1)
        bases = [j[3] for j in jobs[gs[k]:gs[k + 1]]] if route == PAIRS else [ws.PITCH_M]
        if sub:
            depth, nv = ctx.fuse_depth_sub(new["maps"][sl], new["subpix"][sl], bases, ws.F, ws.PS)
        else:
            depth, nv = ctx.fuse_depth(new["maps"][sl], bases, ws.F, ws.PS)
        assert same(new["depth"][k], depth.reshape(ws.H, ws.W)), k
        if route == PAIRS:
            assert same(new["n_valid"][k], nv.reshape(ws.H, ws.W)), k
    assert not same(new["depth"], old["depth"])


@pytest.mark.parametrize("route,check,sub", [(GROUPS, 1, 1), (MIXED, 0, 0), (PAIRS, 0, 1)])
def test_select_1_without_a_fill_is_the_filled_entry(sva, route, check, sub):
    """fill_max_dist 0: n_found is all zero, so wmed_select 1 looks at nothing."""
    want = dict(ALL, want_sub=bool(sub), want_n_valid=route == PAIRS, want_counts=bool(check))
    m = engine(sva)
    try:
        new = smoothed(m, sva, route, check, sub, 1, fill=(0, 1), **want)
        unasked = smoothed(m, sva, route, check, sub, 1, fill=(0, 1), want_maps=True)
        old = filled(m, sva, route, check, sub, fill=(0, 1),
                     **{k: v for k, v in want.items() if k != "want_support"})
    finally:
        m.close()
    for name, plane in old.items():
        assert (plane is None and new[name] is None) or same(new[name], plane), name
    assert old["maps"] is not None and not new["support"].any() and not new["n_found"].any()
    assert same(unasked["maps"], old["maps"]) and same(unasked["depth"], old["depth"])


def test_refusals_write_nothing(sva):
    """The entry's new argument errors come after sva_array_depth_filled's: status,
    message, no kernel launched, canary-filled outputs untouched."""
    INV = sva.SVA_ERR_INVALID_ARG
    counted = ("census", "cost", "sgm_paths", "wta_hv", "fill_scan", "fill_apply", "wmed",
               "fuse_depth")
    rad, sup, sel = ("wmed radius must be 1..15", "wmed min_support must be 1..961",
                     "wmed select must be 0 or 1")
    cases = [
        ("radius_0", rad, dict(r=0)), ("radius_16", rad, dict(r=16)),
        ("min_support_0", sup, dict(ms=0)), ("min_support_962", sup, dict(ms=962)),
        ("select_negative", sel, dict(sel=-1)), ("select_2", sel, dict(sel=2)),
        ("radius_before_min_support", rad, dict(r=16, ms=0, sel=2)),
        ("min_support_before_select", sup, dict(ms=962, sel=2)),
        # the old rules first
        ("fill_mode", "fill mode must be 0..2", dict(fm=3, r=0)),
        ("fill_max_dist", "fill max_dist must be 0..255", dict(fd=256, sel=2)),
        ("check_2", "check must be 0 or 1", dict(check=2, r=16)),
    ]
    w = we.weights(SIGMA)
    m = engine(sva)
    try:
        c0 = m.context(0, 0)
        c0.set_timing(sva.SVA_TIMING_ALL)
        c0.reset_timing()
        jobs, gs, _ = frame_of(sva, GROUPS)
        fr = sva._ArrayFrame(ws.views(), jobs, gs)
        for name, text, ch in cases:
            a = dict(check=0, fd=16, fm=2, r=R, ms=1, sel=0)
            a.update(ch)
            depth = np.full((fr.G, ws.H, ws.W), -7.0, np.float64)
            maps = np.full((fr.G, ws.H, ws.W), 0x5A5A, np.uint16)
            support = np.full((fr.G, ws.H, ws.W), 0x6B6B, np.uint16)
            st = sva.lib.sva_array_depth_smoothed(
                m.h, *fr.head, GROUPS, None, ws.F, ws.PS, 0, sva.SVA_FUSE_MEDIAN,
                depth.ctypes.data, None, None, None, maps.ctypes.data, None, None, None, 0, 1, 2, 8,
                None, None, a["check"], 20, 1, None, a["fd"], 3, a["fm"], None, a["r"],
                w.ctypes.data, a["ms"], a["sel"], support.ctypes.data)
            msg = sva.lib.sva_multi_last_error(m.h).decode()
            assert st == INV and text in msg, (name, st, msg)
            assert (depth == -7.0).all() and (maps == 0x5A5A).all() and (support == 0x6B6B).all()
        assert {k: c0.kernel_time(k)[1] for k in counted} == dict.fromkeys(counted, 0)
        # the engine still works: nine maps of one `invalid` take one launch
        res = smoothed(m, sva, GROUPS, 0, 0, 0, want_maps=True)
        assert c0.kernel_time("wmed")[1] == 1
        base = filled(m, sva, GROUPS, 0, 0, want_maps=True)
    finally:
        m.close()
    assert np.array_equal(res["maps"], we.weighted_median(
        base["maps"], ws.INVALID, R, np.stack(ws.views()), w)[0])
