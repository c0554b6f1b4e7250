"""sva_array_depth_filtered on the engine, on the scene of
tests/cross_scene.py.  The three identities of the entry, bit for bit: with
speckle_max_size 0 it is sva_array_depth_checked (check 1), sva_array_depth_sub
(check 0, sub 1) or the route's own entry (check 0, sub 0); otherwise it is the
stand-alone composition -- the unfiltered frame's maps through sva_cross_check,
sva_filter_speckles and the matching sva_fuse_depth*.  The maps and comp_size
are tests/speckle_expect.py on the expected checked maps, and the filter lowers
the wrong-pixel count of the checked frame to the CPU table's figure."""
import numpy as np
import pytest

import cross_scene as cs
import speckle_expect as sp

pytestmark = pytest.mark.gpu

PAIRS, GROUPS, MIXED = 0, 1, 2
UNIT = [cs.PITCH_M] * 9
SPECKLE = (20, 1)            # max_size, max_diff: the table's
ALL = dict(want_sub=True, want_maps=True, want_costs=True, want_size=True)


def same(a, b):
    return a is not None and b is not None and a.tobytes() == b.tobytes() and a.shape == b.shape


def engine(sva):
    return sva.Multi([0], streams=2, flags=sva.SVA_MULTI_GATHER_PEER)


def frame_of(sva, route, lr_check=0):
    """(jobs, group_start, unit): the scene's groups; on PAIRS two center-style
    groups -- camera 4 against its eight neighbours, camera 0 against its three."""
    if route != PAIRS:
        jobs, gs = cs.jobs(sva, route == MIXED)
        return jobs, gs, UNIT if route == MIXED else None
    jobs, gs = cs.jobs(sva, lr_check=lr_check) if lr_check else cs.jobs(sva)
    mine = jobs[gs[4]:gs[5]] + jobs[gs[0]:gs[1]]
    return mine, [0, gs[5] - gs[4], gs[5] - gs[4] + gs[1] - gs[0]], None


def filtered(m, sva, route, check, sub, speckle, mode=None, lr_check=0, **want):
    jobs, gs, unit = frame_of(sva, route, lr_check)
    return m.array_depth_filtered(
        cs.views(), jobs, gs, cs.F, cs.PS, speckle[0], speckle[1], check=check,
        view_step=cs.VIEW_STEP if check else None, route=route, unit_baseline=unit,
        mode=sva.SVA_FUSE_MEDIAN if mode is None else mode, sub=sub,
        **(cs.CHECK if check else dict(max_diff=-5, min_agree=99, max_conflict=-1)), **want)


@pytest.mark.parametrize("route", [GROUPS, MIXED])
def test_max_size_0_checked_is_the_checked_entry(sva, route):
    jobs, gs, unit = frame_of(sva, route)
    m = engine(sva)
    try:
        for sub in (0, 1):
            new = filtered(m, sva, route, 1, sub, (0, 1), want_counts=True,
                           **dict(ALL, want_sub=bool(sub)))
            old = m.array_depth_checked(cs.views(), jobs, gs, cs.F, cs.PS, cs.VIEW_STEP, route=route,
                                        unit_baseline=unit, sub=sub, want_sub=bool(sub),
                                        want_maps=True, want_costs=True, want_counts=True, **cs.CHECK)
            names = ("depth", "subpix", "maps", "cost_min", "cost_second", "agree", "conflict")
            for name, plane in zip(names, old):
                assert (plane is None and new[name] is None) or same(new[name], plane), (sub, name)
            assert np.array_equal(new["comp_size"], sp.comp_size(old[2], cs.INVALID, 1))
    finally:
        m.close()


@pytest.mark.parametrize("route", [PAIRS, GROUPS, MIXED])
def test_max_size_0_unchecked_is_the_routes_own_entry(sva, route):
    jobs, gs, unit = frame_of(sva, route)
    v = cs.views()
    pair = route == PAIRS
    m = engine(sva)
    try:
        new1 = filtered(m, sva, route, 0, 1, (0, 1), want_n_valid=pair, **ALL)
        osub = m.array_depth_sub(v, jobs, gs, cs.F, cs.PS, route=route, unit_baseline=unit,
                                 want_sub=True, want_maps=True, want_costs=True)
        mode = sva.SVA_FUSE_MIN_COST if pair else sva.SVA_FUSE_MEDIAN
        new0 = filtered(m, sva, route, 0, 0, (0, 1), mode=mode, want_n_valid=pair, want_winner=pair,
                        **dict(ALL, want_sub=False))
        if pair:
            depth, nv, win, maps, cmin, csec = m.array_depth_conf(v, jobs, gs, cs.F, cs.PS, 0, mode,
                                                                  want_maps=True, want_costs=True)
        elif route == GROUPS:
            depth, maps, cmin, csec = m.array_depth_mb(v, jobs, gs, cs.F, cs.PS, 0, want_maps=True,
                                                       want_costs=True)
        else:
            depth, maps, cmin, csec = m.array_depth_mixed(v, jobs, gs, unit, cs.F, cs.PS, 0,
                                                          want_maps=True, want_costs=True)
    finally:
        m.close()
    for name, plane in zip(("depth", "n_valid", "winner", "subpix", "maps", "cost_min", "cost_second"),
                           osub):
        if plane is not None and (pair or name not in ("n_valid", "winner")):
            assert same(new1[name], plane), name
    assert same(new0["depth"], depth) and same(new0["maps"], maps)
    assert same(new0["cost_min"], cmin) and same(new0["cost_second"], csec)
    if pair:
        assert same(new0["n_valid"], nv) and same(new0["winner"], win)
    assert np.array_equal(new0["comp_size"], sp.comp_size(maps, cs.INVALID, 1))


@pytest.mark.parametrize("route", [GROUPS, MIXED])
def test_checked_and_filtered_groups(sva, ctx, route):
    """check 1, sub 1: the maps and comp_size are speckle_expect on the expected
    checked maps; subpix and depth are the composition's, bit for bit."""
    jobs, gs, unit = frame_of(sva, route)
    m = engine(sva)
    try:
        new = filtered(m, sva, route, 1, 1, SPECKLE, want_counts=True, **ALL)
        bare = filtered(m, sva, route, 1, 1, SPECKLE)
        raw = m.array_depth_sub(cs.views(), jobs, gs, cs.F, cs.PS, route=route, unit_baseline=unit,
                                want_sub=True, want_maps=True, want_costs=True)
    finally:
        m.close()
    eo, _, ea, ec = cs.checked(route == MIXED, **cs.CHECK)
    fo, _, size = sp.filter_speckles(eo, cs.INVALID, *SPECKLE)
    assert np.array_equal(new["maps"], fo) and np.array_equal(new["comp_size"], size)
    assert np.array_equal(new["agree"], ea) and np.array_equal(new["conflict"], ec)
    assert ((fo == cs.INVALID) & (eo != cs.INVALID)).any()
    # the composition on the unfiltered frame's own planes
    c_maps, c_sub, _, _ = ctx.cross_check(raw[4], cs.VIEW_STEP, raw[3], cs.INVALID, **cs.CHECK)
    f_maps, f_sub, f_size = ctx.filter_speckles(c_maps, *SPECKLE, subpix=c_sub)
    assert same(new["maps"], f_maps) and same(new["subpix"], f_sub) and same(new["comp_size"], f_size)
    assert np.array_equal(np.isnan(f_sub), f_maps == cs.INVALID)
    for g in range(9):
        depth = ctx.fuse_depth_sub(f_maps[g][None], f_sub[g][None], [cs.PITCH_M], cs.F, cs.PS)[0]
        assert same(new["depth"][g], depth.reshape(cs.H, cs.W)), g
    assert same(new["cost_min"], raw[5]) and same(new["cost_second"], raw[6])
    assert same(bare["depth"], new["depth"])
    assert all(bare[k] is None for k in bare if k != "depth")


@pytest.mark.parametrize("mode_name", ["median", "min_cost"])
def test_filtered_pairs(sva, ctx, mode_name):
    """check 0 on SVA_ARRAY_PAIRS with per-pair lr_check: every pair's map is
    filtered, then each group's maps are fused by `mode`."""
    mode = sva.SVA_FUSE_MEDIAN if mode_name == "median" else sva.SVA_FUSE_MIN_COST
    by_cost = mode != sva.SVA_FUSE_MEDIAN
    jobs, gs, _ = frame_of(sva, PAIRS, lr_check=1)
    m = engine(sva)
    try:
        new = filtered(m, sva, PAIRS, 0, 0, SPECKLE, mode=mode, lr_check=1, want_n_valid=True,
                       want_winner=by_cost, **dict(ALL, want_sub=False))
        raw = m.array_depth_conf(cs.views(), jobs, gs, cs.F, cs.PS, 0, mode, want_maps=True,
                                 want_costs=True)
    finally:
        m.close()
    maps, cmin, csec = raw[3], raw[4], raw[5]
    fo, _, size = sp.filter_speckles(maps, cs.INVALID, *SPECKLE)
    assert ((fo == cs.INVALID) & (maps != cs.INVALID)).any()
    assert np.array_equal(new["maps"], fo) and np.array_equal(new["comp_size"], size)
    assert same(new["cost_min"], cmin) and same(new["cost_second"], csec)
    f_maps = ctx.filter_speckles(maps, *SPECKLE, want_size=False)[0]
    assert same(f_maps, fo)
    for g in range(len(gs) - 1):
        sl = slice(gs[g], gs[g + 1])
        bases = [j[3] for j in jobs[sl]]
        if by_cost:
            depth, nv, win = ctx.fuse_depth_conf(f_maps[sl], cmin[sl], csec[sl], bases, cs.F, cs.PS,
                                                 cs.INVALID, mode)
            assert same(new["winner"][g], win.reshape(cs.H, cs.W)), g
        else:
            depth, nv = ctx.fuse_depth(f_maps[sl], bases, cs.F, cs.PS)
        assert same(new["depth"][g], depth.reshape(cs.H, cs.W)), g
        assert same(new["n_valid"][g], nv.reshape(cs.H, cs.W)), g
    assert not same(new["depth"], raw[0])


def test_quality_on_the_gpu_maps(sva):
    """The GPU's maps give the CPU table's counts, and the
    filter leaves strictly fewer wrong pixels than the checked frame."""
    jobs, gs, _ = frame_of(sva, GROUPS)
    m = engine(sva)
    try:
        checked = m.array_depth_checked(cs.views(), jobs, gs, cs.F, cs.PS, cs.VIEW_STEP,
                                        want_maps=True, **cs.CHECK)[2]
        after = filtered(m, sva, GROUPS, 1, 0, SPECKLE, want_maps=True)["maps"]
        alone = filtered(m, sva, GROUPS, 0, 0, SPECKLE, want_maps=True)["maps"]
    finally:
        m.close()
    eo = cs.checked(**cs.CHECK)[0]
    q_checked, q_after, q_alone = cs.quality(checked), cs.quality(after), cs.quality(alone)
    print("checked %s, checked + filtered %s, filtered alone %s" % (q_checked, q_after, q_alone))
    assert q_checked == cs.quality(eo)
    assert q_after == cs.quality(sp.filter_speckles(eo, cs.INVALID, *SPECKLE)[0])
    assert q_alone == cs.quality(sp.filter_speckles(cs.matched()[0], cs.INVALID, *SPECKLE)[0])
    assert q_after[0] < q_checked[0]


def test_refusals_write_nothing(sva):
    """The entry's new argument errors: status, message, no kernel launched,
    canary-filled outputs untouched."""
    INV, UNS = sva.SVA_ERR_INVALID_ARG, sva.SVA_ERR_UNSUPPORTED
    counted = ("census", "cost", "sgm_paths", "wta_hv", "cross_check", "speckle_label",
               "speckle_apply", "fuse_depth")
    # (name, status, message, arguments that differ from a valid check = 0 GROUPS call)
    cases = [
        ("check_2", INV, "check must be 0 or 1", dict(check=2)),
        ("check_negative", INV, "check must be 0 or 1", dict(check=-1)),
        ("sub_2", INV, "sub must be 0 or 1", dict(sub=2)),
        ("agree", INV, "agree and conflict need check = 1", dict(agree=True)),
        ("conflict", INV, "agree and conflict need check = 1", dict(conflict=True)),
        ("subpix_without_sub", INV, "subpix needs sub = 1", dict(subpix=True)),
        ("max_size", INV, "speckle max_size must be >= 0", dict(ms=-1)),
        ("max_diff", INV, "speckle max_diff must be >= 0", dict(md=-1)),
        ("pairs_checked", UNS, "needs a group route", dict(route=PAIRS, check=1, steps=True)),
        ("mode_on_groups", INV, "SVA_FUSE_MEDIAN only", dict(mode=sva.SVA_FUSE_MIN_COST)),
        ("check_2_and_max_size", INV, "check must be 0 or 1", dict(check=2, ms=-1)),
        ("agree_and_max_diff", INV, "agree and conflict need check = 1", dict(agree=True, md=-1)),
    ]
    m = engine(sva)
    try:
        c0 = m.context(0, 0)
        c0.set_timing(sva.SVA_TIMING_ALL)
        c0.reset_timing()
        for name, status, text, ch in cases:
            a = dict(route=GROUPS, check=0, sub=0, agree=False, conflict=False, subpix=False, ms=20,
                     md=1, mode=sva.SVA_FUSE_MEDIAN, steps=False)
            a.update(ch)
            jobs, gs, unit = frame_of(sva, a["route"])
            fr = sva._ArrayFrame(cs.views(), jobs, gs)
            nj = len(jobs) if a["route"] == PAIRS else fr.G
            depth = np.full((fr.G, cs.H, cs.W), -7.0, np.float64)
            subp = np.full((nj, cs.H, cs.W), -7.0, np.float32)
            maps = np.full((nj, cs.H, cs.W), 0x5A5A, np.uint16)
            size = np.full((nj, cs.H, cs.W), 0x6B6B6B6B, np.uint32)
            counts = np.full((2, fr.G, cs.H, cs.W), 0xEE, np.uint8)
            st = sva.lib.sva_array_depth_filtered(
                m.h, *fr.head, a["route"], None, cs.F, cs.PS, 0, a["mode"], depth.ctypes.data, None,
                None, subp.ctypes.data if a["subpix"] else None, maps.ctypes.data, None, None,
                sva._steps(cs.VIEW_STEP, 9) if a["steps"] else None, a["sub"], 1, 2, 8,
                counts[0].ctypes.data if a["agree"] else None,
                counts[1].ctypes.data if a["conflict"] else None, a["check"], a["ms"], a["md"],
                size.ctypes.data)
            msg = sva.lib.sva_multi_last_error(m.h).decode()
            assert st == status and text in msg, (name, st, msg)
            assert (depth == -7.0).all() and (subp == -7.0).all() and (maps == 0x5A5A).all(), name
            assert (size == 0x6B6B6B6B).all() and (counts == 0xEE).all(), name
        assert {k: c0.kernel_time(k)[1] for k in counted} == dict.fromkeys(counted, 0)
        # the engine still works; a filtered frame of nine maps with one `invalid` is one call
        res = filtered(m, sva, GROUPS, 0, 0, SPECKLE, want_maps=True)
        assert c0.kernel_time("speckle_label")[1] == 1 and c0.kernel_time("speckle_merge")[1] == 1
        assert c0.kernel_time("cross_check")[1] == 0
    finally:
        m.close()
    assert np.array_equal(res["maps"],
                          sp.filter_speckles(cs.matched()[0], cs.INVALID, *SPECKLE)[0])
