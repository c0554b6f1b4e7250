"""sva_array_depth_filled on the engine, on the scene of
tests/cross_scene.py.  Bit for bit: with fill_max_dist 0 it is
sva_array_depth_filtered; otherwise it is the stand-alone composition -- the
filtered frame's maps through sva_fill_holes, then the matching
sva_fuse_depth*.  n_found is the stand-alone one, the maps are
tests/fill_expect.py's, and the new refusals come after the old ones."""
import os
import re

import numpy as np
import pytest

import cross_scene as cs
import fill_expect as fe

pytestmark = pytest.mark.gpu

PAIRS, GROUPS, MIXED = 0, 1, 2
UNIT = [cs.PITCH_M] * 9
SPECKLE = (20, 1)
FILL = (16, 3)               # max_dist, min_found: the quality table's
_TUNING = os.path.join(os.path.dirname(__file__), "..", "stereovisionarray_amd", "csrc",
                       "sva_tuning.h")
CHUNK = int(re.search(r"kFillFrameMaps = (\d+)", open(_TUNING).read()).group(1))
ALL = dict(want_sub=True, want_maps=True, want_costs=True, want_size=True)


def same(a, b):
    return a is not None and b is not None and a.tobytes() == b.tobytes() and a.shape == b.shape


def engine(sva):
    return sva.Multi([0], streams=2, flags=sva.SVA_MULTI_GATHER_PEER)


def frame_of(sva, route):
    """(jobs, group_start, unit): the scene's groups; on PAIRS two center-style
    groups -- camera 4 against its eight neighbours, camera 0 against its three."""
    if route != PAIRS:
        jobs, gs = cs.jobs(sva, route == MIXED)
        return jobs, gs, UNIT if route == MIXED else None
    jobs, gs = cs.jobs(sva)
    mine = jobs[gs[4]:gs[5]] + jobs[gs[0]:gs[1]]
    return mine, [0, gs[5] - gs[4], gs[5] - gs[4] + gs[1] - gs[0]], None


def frame_args(sva, route, check, sub):
    jobs, gs, unit = frame_of(sva, route)
    return (cs.views(), jobs, gs, cs.F, cs.PS), dict(
        check=check, view_step=cs.VIEW_STEP if check else None, route=route, unit_baseline=unit,
        mode=sva.SVA_FUSE_MEDIAN, sub=sub, **(cs.CHECK if check else {}))


def filled(m, sva, route, check, sub, fill, fill_mode, speckle=SPECKLE, **want):
    pos, kw = frame_args(sva, route, check, sub)
    return m.array_depth_filled(*pos, fill[0], fill[1], fill_mode, speckle_max_size=speckle[0],
                                speckle_max_diff=speckle[1], **kw, **want)


def filtered(m, sva, route, check, sub, speckle=SPECKLE, **want):
    pos, kw = frame_args(sva, route, check, sub)
    return m.array_depth_filtered(*pos, speckle[0], speckle[1], **kw, **want)


@pytest.mark.parametrize("route,check,sub", [(GROUPS, 1, 1), (MIXED, 0, 0), (PAIRS, 0, 1)])
def test_max_dist_0_is_the_filtered_entry(sva, route, check, sub):
    pair = route == PAIRS
    want = dict(ALL, want_sub=bool(sub), want_counts=bool(check), want_n_valid=pair)
    m = engine(sva)
    try:
        new = filled(m, sva, route, check, sub, (0, 8), sva.SVA_FILL_MIN, want_found=True, **want)
        old = filtered(m, sva, route, check, sub, **want)
    finally:
        m.close()
    for name, plane in old.items():
        assert (plane is None and new[name] is None) or same(new[name], plane), name
    assert old["maps"] is not None and old["depth"] is not None and old["comp_size"] is not None
    assert new["n_found"].shape == old["maps"].shape and not new["n_found"].any()


@pytest.mark.parametrize("fill_mode", fe.MODES)
def test_checked_filtered_and_filled_groups(sva, ctx, fill_mode):
    """A group route with check 1, sub 1: maps, subpix and n_found are the
    stand-alone fill of the filtered frame's, depth the fusion of those."""
    m = engine(sva)
    try:
        new = filled(m, sva, GROUPS, 1, 1, FILL, fill_mode, want_counts=True, want_found=True, **ALL)
        bare = filled(m, sva, GROUPS, 1, 1, FILL, fill_mode)
        old = filtered(m, sva, GROUPS, 1, 1, want_counts=True, **ALL)
    finally:
        m.close()
    f_maps, f_sub, f_found = ctx.fill_holes(old["maps"], FILL[0], FILL[1], fill_mode,
                                            subpix=old["subpix"])
    assert same(new["maps"], f_maps) and same(new["subpix"], f_sub)
    assert same(new["n_found"], f_found)
    eo, es, ef, was_filled = fe.fill_holes(old["maps"], cs.INVALID, FILL[0], FILL[1], fill_mode,
                                           old["subpix"])
    assert np.array_equal(new["maps"], eo) and np.array_equal(new["n_found"], ef)
    assert same(new["subpix"], es) and was_filled.sum() > 1000
    assert not np.isnan(new["subpix"][was_filled]).any()
    for g in range(9):
        depth = ctx.fuse_depth_sub(f_maps[g][None], f_sub[g][None], [cs.PITCH_M], cs.F, cs.PS)[0]
        assert same(new["depth"][g], depth.reshape(cs.H, cs.W)), g
    assert not same(new["depth"], old["depth"])
    # the planes the fill does not touch
    for name in ("cost_min", "cost_second", "agree", "conflict", "comp_size"):
        assert same(new[name], old[name]), name
    assert same(bare["depth"], new["depth"])
    assert all(bare[k] is None for k in bare if k != "depth")


@pytest.mark.parametrize("sub", [0, 1])
def test_filled_pairs(sva, ctx, sub):
    """check 0 on SVA_ARRAY_PAIRS, MEDIAN: every pair's map is filled after the
    speckle filter, then each group's maps are fused."""
    jobs, gs, _ = frame_of(sva, PAIRS)
    want = dict(ALL, want_sub=bool(sub), want_n_valid=True)
    m = engine(sva)
    try:
        new = filled(m, sva, PAIRS, 0, sub, FILL, sva.SVA_FILL_SECOND, want_found=True, **want)
        old = filtered(m, sva, PAIRS, 0, sub, **want)
    finally:
        m.close()
    f_maps, f_sub, f_found = ctx.fill_holes(old["maps"], FILL[0], FILL[1], sva.SVA_FILL_SECOND,
                                            subpix=old["subpix"])
    assert same(new["maps"], f_maps) and same(new["n_found"], f_found)
    assert np.array_equal(f_maps, fe.fill_holes(old["maps"], cs.INVALID, FILL[0], FILL[1],
                                                fe.SECOND)[0])
    assert (f_maps != old["maps"]).sum() > 1000
    if sub:
        assert same(new["subpix"], f_sub)
    else:
        assert new["subpix"] is None and f_sub is None
    for g in range(len(gs) - 1):
        sl = slice(gs[g], gs[g + 1])
        bases = [j[3] for j in jobs[sl]]
        if sub:
            depth, nv = ctx.fuse_depth_sub(f_maps[sl], f_sub[sl], bases, cs.F, cs.PS)
        else:
            depth, nv = ctx.fuse_depth(f_maps[sl], bases, cs.F, cs.PS)
        assert same(new["depth"][g], depth.reshape(cs.H, cs.W)), g
        assert same(new["n_valid"][g], nv.reshape(cs.H, cs.W)), g
    assert not same(new["depth"], old["depth"])
    assert same(new["cost_min"], old["cost_min"]) and same(new["cost_second"], old["cost_second"])
    assert same(new["comp_size"], old["comp_size"])


def test_refusals_write_nothing(sva):
    """The entry's new argument errors come after sva_array_depth_filtered's:
    status, message, no kernel launched, canary-filled outputs untouched."""
    INV = sva.SVA_ERR_INVALID_ARG
    counted = ("census", "cost", "sgm_paths", "wta_hv", "speckle_label", "speckle_apply",
               "fill_scan", "fill_apply", "fuse_depth")
    dist, found, mode = ("fill max_dist must be 0..255", "fill min_found must be 1..8",
                         "fill mode must be 0..2")
    # (name, message, arguments that differ from a valid check = 0 GROUPS call)
    cases = [
        ("max_dist_negative", dist, dict(fd=-1)), ("max_dist_256", dist, dict(fd=256)),
        ("min_found_0", found, dict(ff=0)), ("min_found_9", found, dict(ff=9)),
        ("mode_negative", mode, dict(fm=-1)), ("mode_3", mode, dict(fm=3)),
        ("max_dist_before_min_found", dist, dict(fd=256, ff=0, fm=3)),
        ("min_found_before_mode", found, dict(ff=0, fm=3)),
        # the old rules first
        ("sub_2", "sub must be 0 or 1", dict(sub=2, fd=256)),
        ("check_2", "check must be 0 or 1", dict(check=2, fd=256)),
        ("speckle_max_size", "speckle max_size must be >= 0", dict(ms=-1, fd=256)),
        ("speckle_max_diff", "speckle max_diff must be >= 0", dict(md=-1, ff=0)),
        ("mode_on_groups", "SVA_FUSE_MEDIAN only", dict(fuse=sva.SVA_FUSE_MIN_COST, fm=3)),
    ]
    m = engine(sva)
    try:
        c0 = m.context(0, 0)
        c0.set_timing(sva.SVA_TIMING_ALL)
        c0.reset_timing()
        jobs, gs, _ = frame_of(sva, GROUPS)
        fr = sva._ArrayFrame(cs.views(), jobs, gs)
        for name, text, ch in cases:
            a = dict(check=0, sub=0, ms=20, md=1, fuse=sva.SVA_FUSE_MEDIAN, fd=16, ff=3, fm=1)
            a.update(ch)
            depth = np.full((fr.G, cs.H, cs.W), -7.0, np.float64)
            maps = np.full((fr.G, cs.H, cs.W), 0x5A5A, np.uint16)
            size = np.full((fr.G, cs.H, cs.W), 0x6B6B6B6B, np.uint32)
            nf = np.full((fr.G, cs.H, cs.W), 0xEE, np.uint8)
            st = sva.lib.sva_array_depth_filled(
                m.h, *fr.head, GROUPS, None, cs.F, cs.PS, 0, a["fuse"], depth.ctypes.data, None,
                None, None, maps.ctypes.data, None, None, None, a["sub"], 1, 2, 8, None, None,
                a["check"], a["ms"], a["md"], size.ctypes.data, a["fd"], a["ff"], a["fm"],
                nf.ctypes.data)
            msg = sva.lib.sva_multi_last_error(m.h).decode()
            assert st == INV and text in msg, (name, st, msg)
            assert (depth == -7.0).all() and (maps == 0x5A5A).all(), name
            assert (size == 0x6B6B6B6B).all() and (nf == 0xEE).all(), name
        assert {k: c0.kernel_time(k)[1] for k in counted} == dict.fromkeys(counted, 0)
        # the engine still works; nine maps with one `invalid` are filled in
        # calls of at most kFillFrameMaps maps
        res = filled(m, sva, GROUPS, 0, 0, FILL, sva.SVA_FILL_MEDIAN, want_maps=True)
        calls = -(-9 // CHUNK)
        assert c0.kernel_time("fill_scan")[1] == calls and c0.kernel_time("fill_apply")[1] == calls
        base = filtered(m, sva, GROUPS, 0, 0, want_maps=True)
    finally:
        m.close()
    assert np.array_equal(res["maps"], fe.fill_holes(base["maps"], cs.INVALID, FILL[0], FILL[1],
                                                     fe.MEDIAN)[0])
