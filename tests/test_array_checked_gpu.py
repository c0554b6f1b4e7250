"""sva_array_depth_checked on the engine, on the scene of
tests/cross_scene.py: nine reference cameras, each matched multi-baseline
against its neighbours, and the cross-view check between their maps before
depth.  The maps and count planes are the CPU oracle's maps through
tests/cross_expect.py byte for byte, depth is the fusion of the returned maps,
the identity thresholds give the unchecked entries' outputs, and the check
removes more than half of the wrong pixels for under 2 % of the correct ones."""
import numpy as np
import pytest

import cross_expect as ce
import cross_scene as cs
import sub_expect as se

pytestmark = pytest.mark.gpu

GROUPS, MIXED = 1, 2
SUB_TOL = 1e-5
UNIT = [cs.PITCH_M] * 9
IDENTITY = dict(max_diff=1, min_agree=0, max_conflict=31)


def same32(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same64(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def run(m, sva, route=GROUPS, sub=0, check=cs.CHECK, **want):
    jobs, gs = cs.jobs(sva, route == MIXED)
    return m.array_depth_checked(cs.views(), jobs, gs, cs.F, cs.PS, cs.VIEW_STEP, route=route,
                                 unit_baseline=UNIT if route == MIXED else None, sub=sub, **check,
                                 **want)


def engine(sva):
    return sva.Multi([0], streams=2, flags=sva.SVA_MULTI_GATHER_PEER)


def check_frame(res, oracle, route, sub, thresholds):
    depth, subp, maps, cmin, csec, agree, conflict = res
    eo, es, ea, ec = cs.checked(route == MIXED, **thresholds)
    assert np.array_equal(maps, eo), int((maps != eo).sum())
    assert np.array_equal(agree, ea) and np.array_equal(conflict, ec)
    if sub:
        assert np.array_equal(np.isnan(subp), np.isnan(es))
        assert np.array_equal(np.isnan(subp), maps == cs.INVALID)
        keep = ~np.isnan(es)
        assert np.max(np.abs(subp[keep] - es[keep])) <= SUB_TOL
    else:
        assert subp is None
    for g in range(9):
        if sub:
            exp = se.fuse_expect(maps[g][None], subp[g][None], None, None, [cs.PITCH_M], cs.F,
                                 cs.PS, cs.INVALID, se.FUSE_MEDIAN)[0]
        else:
            exp, _ = oracle.fuse_depth(maps[g][None], [cs.PITCH_M], cs.F, cs.PS)
        assert same64(depth[g], exp), g
        assert (depth[g][maps[g] == cs.INVALID] == 0).all() and (depth[g] > 0).any()


@pytest.mark.parametrize("sub", [0, 1])
def test_groups(sva, oracle, sub):
    m = engine(sva)
    try:
        res = run(m, sva, GROUPS, sub, want_sub=bool(sub), want_maps=True, want_counts=True)
        bare = run(m, sva, GROUPS, sub)
    finally:
        m.close()
    check_frame(res, oracle, GROUPS, sub, cs.CHECK)
    # the check rejected something, and a caller who asks for no plane gets the same depth
    before = cs.matched()[0]
    assert ((res[2] == cs.INVALID) & (before != cs.INVALID)).any()
    assert same64(bare[0], res[0]) and all(p is None for p in bare[1:])


def test_groups_mixed(sva, oracle):
    """Every reference camera against all eight others: the corners' far pairs
    are at 2/1 of the unit baseline."""
    pairs, gs = cs.groups(True)
    assert {k for *_, k in pairs[gs[0]:gs[1]]} == {1, 2} and gs[-1] == 72
    m = engine(sva)
    try:
        res = run(m, sva, MIXED, 1, want_sub=True, want_maps=True, want_counts=True)
        plain = run(m, sva, MIXED, 0, want_maps=True, want_counts=True)
    finally:
        m.close()
    check_frame(res, oracle, MIXED, 1, cs.CHECK)
    check_frame(plain, oracle, MIXED, 0, cs.CHECK)


@pytest.mark.parametrize("route", [GROUPS, MIXED])
def test_identity_equals_the_unchecked_entries(sva, route):
    """min_agree 0 and max_conflict 31 reject nothing: every shared output is
    that of sva_array_depth_mb / _mixed (sub 0) or sva_array_depth_sub (sub 1)."""
    jobs, gs = cs.jobs(sva, route == MIXED)
    v = cs.views()
    m = engine(sva)
    try:
        c0 = run(m, sva, route, 0, IDENTITY, want_maps=True, want_costs=True, want_counts=True)
        c1 = run(m, sva, route, 1, IDENTITY, want_sub=True, want_maps=True, want_costs=True)
        if route == GROUPS:
            old = m.array_depth_mb(v, jobs, gs, cs.F, cs.PS, 0, want_maps=True, want_costs=True)
        else:
            old = m.array_depth_mixed(v, jobs, gs, UNIT, cs.F, cs.PS, 0, want_maps=True,
                                      want_costs=True)
        osub = m.array_depth_sub(v, jobs, gs, cs.F, cs.PS, route=route,
                                 unit_baseline=UNIT if route == MIXED else None, want_sub=True,
                                 want_maps=True, want_costs=True)
    finally:
        m.close()
    depth, maps, cmin, csec = old
    assert same64(c0[0], depth) and c0[2].tobytes() == maps.tobytes()
    assert c0[3].tobytes() == cmin.tobytes() and c0[4].tobytes() == csec.tobytes()
    assert same64(c1[0], osub[0]) and same32(c1[1], osub[3])
    for k, j in ((2, 4), (3, 5), (4, 6)):
        assert c1[k].tobytes() == osub[j].tobytes()
    # the counts are still those of the rule
    ea, ec = ce.counts(maps, cs.VIEW_STEP, cs.INVALID, 1)
    assert np.array_equal(c0[5], ea) and np.array_equal(c0[6], ec)


def test_quality():
    """Wrong = valid and |d - truth| > 1 over [12:-12, 12:-12] of all nine views,
    on the EXPECTED maps (test_groups holds the GPU to them byte for byte): the
    check at max_diff 1, min_agree 2, max_conflict 8 leaves at most half of the
    wrong pixels and at least 98 % of the correct ones.  The CPU oracle gives
    1444 -> 552 wrong and 65948 -> 65591 correct."""
    wrong0, right0 = cs.quality(cs.matched()[0])
    wrong1, right1 = cs.quality(cs.checked(**cs.CHECK)[0])
    print("wrong %d -> %d, correct %d -> %d" % (wrong0, wrong1, right0, right1))
    assert wrong0 > 0
    assert wrong1 <= 0.5 * wrong0
    assert right1 >= 0.98 * right0


def test_quality_on_the_gpu_maps(sva):
    m = engine(sva)
    try:
        before = m.array_depth_mb(cs.views(), *cs.jobs(sva), cs.F, cs.PS, 0, want_maps=True)[1]
        after = run(m, sva, GROUPS, 0, want_maps=True)[2]
    finally:
        m.close()
    (wrong0, right0), (wrong1, right1) = cs.quality(before), cs.quality(after)
    print("wrong %d -> %d, correct %d -> %d" % (wrong0, wrong1, right0, right1))
    assert wrong1 <= 0.5 * wrong0
    assert right1 >= 0.98 * right0


def test_across_devices(sva):
    n = min(sva.device_count(), 4)
    if n < 2:
        pytest.skip("needs >= 2 HIP devices")
    want = dict(want_sub=True, want_maps=True, want_costs=True, want_counts=True)
    one = engine(sva)
    try:
        ref = {route: run(one, sva, route, 1, **want) for route in (GROUPS, MIXED)}
    finally:
        one.close()
    for flags in (sva.SVA_MULTI_GATHER_RCCL, sva.SVA_MULTI_GATHER_PEER):
        m = sva.Multi(list(range(n)), streams=2, flags=flags)
        try:
            got = {route: run(m, sva, route, 1, **want) for route in (GROUPS, MIXED)}
        finally:
            m.close()
        for route in got:
            for a, b in zip(got[route], ref[route]):
                assert a.tobytes() == b.tobytes()


def test_refusals_write_nothing(sva):
    """Every new argument error through the entry: the status, the message, no
    kernel launched and canary-filled outputs untouched."""
    INV, UNS = sva.SVA_ERR_INVALID_ARG, sva.SVA_ERR_UNSUPPORTED
    v = cs.views()
    jobs, gs = cs.jobs(sva)
    mjobs, mgs = cs.jobs(sva, True)
    counted = ("census", "cost", "cost_fuse", "sgm_paths", "wta_hv", "cross_check", "fuse_depth",
               "fuse_depth_sub")

    def edit(jobs, which, **fields):
        """jobs with the pairs `which` rebuilt: params fields, or ref / other / baseline."""
        out = list(jobs)
        for j in which:
            a, b, p, base = out[j]
            q = sva.default_params(D=p.D, dmin=p.dmin, dir=p.dir, dir_y=p.dir_y, invalid=p.invalid)
            for k, val in fields.items():
                if k not in ("ref", "other", "baseline"):
                    setattr(q, k, val)
            out[j] = (fields.get("ref", a), fields.get("other", b), q, fields.get("baseline", base))
        return out

    g1 = range(gs[1], gs[2])
    moved = list(cs.VIEW_STEP)
    moved[8] = (-2, -1)
    far = [(x + 255, y) for x, y in cs.VIEW_STEP]
    line_steps = [(16 - c, 0) for c in range(34)]
    line_jobs = [(g, g + 1, sva.default_params(D=cs.D, dir=-1, dir_y=0), cs.PITCH_M)
                 for g in range(33)]
    step_x = sva.default_params(D=cs.D, dir=-1, dir_y=0)
    # (name, status, message, arguments that differ from the valid call)
    cases = [
        ("pair_route", UNS, "needs a group route", dict(route=0)),
        ("unknown_route", INV, "unknown route", dict(route=3)),
        ("sub_2", INV, "sub must be 0 or 1", dict(sub=2)),
        ("mode", INV, "SVA_FUSE_MEDIAN only", dict(mode=sva.SVA_FUSE_MIN_COST)),
        ("lr_check", UNS, "no L/R check", dict(jobs=edit(jobs, [3], lr_check=1))),
        ("subpix_without_sub", INV, "subpix needs sub = 1", dict(sub=0, subpix=True)),
        ("null_view_step", INV, "null view_step", dict(view_step=None)),
        ("same_ref", INV, "groups 0 and 1 share ref",
         dict(jobs=jobs[:gs[1]] + jobs[:gs[1]] + jobs[gs[2]:],
              gs=[0, gs[1], 2 * gs[1]] + [g + 2 * gs[1] - gs[2] for g in gs[3:]])),
        ("invalid_differs", INV, "params.invalid of group 1 differs",
         dict(jobs=edit(jobs, g1, invalid=0))),
        ("scale_differs", INV, "the depth scale of group 1 differs",
         dict(jobs=edit(jobs, g1, baseline=2 * cs.PITCH_M))),
        ("scale_differs_mixed", INV, "the depth scale of group 1 differs",
         dict(route=MIXED, jobs=mjobs, gs=mgs, unit=[1.0, 2.0] + [1.0] * 7)),
        ("geometry", INV, "contradicts view_step", dict(view_step=moved)),
        ("step_range", INV, "view_step components must be -255..255", dict(view_step=far)),
        ("max_diff", INV, "max_diff must be >= 0", dict(max_diff=-1)),
        ("min_agree", INV, "min_agree must be 0..31", dict(min_agree=32)),
        ("max_conflict", INV, "max_conflict must be 0..31", dict(max_conflict=-1)),
        ("null_view_step_and_max_diff", INV, "null view_step", dict(view_step=None, max_diff=-1)),
        # 34 cameras on a line, camera g against its neighbour: 33 groups
        ("groups_33", UNS, "the cross-view check takes 1..32 groups",
         dict(views=[v[0]] * 34, jobs=line_jobs, gs=list(range(34)), view_step=line_steps)),
        # two reference cameras at one position, each against camera 1 with a consistent step
        ("equal_view_step", INV, "two views have the same view_step",
         dict(views=v[:3], jobs=[(0, 1, step_x, cs.PITCH_M), (2, 1, step_x, cs.PITCH_M)],
              gs=[0, 1, 2], view_step=[(0, 0), (-1, 0), (0, 0)])),
    ]
    m = engine(sva)
    try:
        c0 = m.context(0, 0)
        c0.set_timing(sva.SVA_TIMING_ALL)
        c0.reset_timing()
        for name, status, text, ch in cases:
            a = dict(route=GROUPS, sub=1, mode=sva.SVA_FUSE_MEDIAN, jobs=jobs, gs=gs, unit=None,
                     view_step=cs.VIEW_STEP, subpix=True, views=v, **cs.CHECK)
            a.update(ch)
            G = len(a["gs"]) - 1
            shape = (G, cs.H, cs.W)
            if a["route"] == MIXED and a["unit"] is None:
                a["unit"] = UNIT
            fr = sva._ArrayFrame(a["views"], a["jobs"], a["gs"])
            depth = np.full(shape, -7.0, np.float64)
            subp = np.full(shape, -7.0, np.float32)
            maps, cmin, csec = (np.full(shape, 0x5A5A, np.uint16) for _ in range(3))
            agree, conflict = (np.full(shape, 0xEE, np.uint8) for _ in range(2))
            unit = None if a["unit"] is None else (sva.ct.c_double * G)(*a["unit"])
            st = sva.lib.sva_array_depth_checked(
                m.h, *fr.head, a["route"], unit, cs.F, cs.PS, 0, a["mode"], depth.ctypes.data, None,
                None, subp.ctypes.data if a["subpix"] else None, maps.ctypes.data,
                cmin.ctypes.data, csec.ctypes.data, sva._steps(a["view_step"], len(a["views"])), a["sub"],
                a["max_diff"], a["min_agree"], a["max_conflict"], agree.ctypes.data,
                conflict.ctypes.data)
            msg = sva.lib.sva_multi_last_error(m.h).decode()
            assert st == status and text in msg, (name, st, msg)
            assert (depth == -7.0).all() and (subp == -7.0).all(), name
            assert all((p == 0x5A5A).all() for p in (maps, cmin, csec)), name
            assert (agree == 0xEE).all() and (conflict == 0xEE).all(), name
        assert {k: c0.kernel_time(k)[1] for k in counted} == dict.fromkeys(counted, 0)
        # the engine still works, and a valid frame launches the check once
        res = run(m, sva, GROUPS, 0, want_maps=True)
        assert c0.kernel_time("cross_check")[1] == 1
    finally:
        m.close()
    assert np.array_equal(res[2], cs.checked(**cs.CHECK)[0])
