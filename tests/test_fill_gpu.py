"""sva_fill_holes / sva_fill_holes_d on the GPU: every
output byte against tests/fill_expect.py, at the frame sizes and distances
around the scan's segment length, on random maps of every hole share, an
all-valid map and single sources; the distance limit; the tie-breaks; map
independence; in place; absent planes; 2-byte aligned views; workspace reuse;
the host twin; the refusals with nothing written."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import fill_expect as fe

pytestmark = pytest.mark.gpu

INVALID = 0xFFFF
_TUNING = os.path.join(os.path.dirname(__file__), "..", "stereovisionarray_amd", "csrc",
                       "sva_tuning.h")
S = int(re.search(r"kFillSegment = (\d+)", open(_TUNING).read()).group(1))
# (W, H): one pixel; a row and a column one pixel longer than a segment; the
# segment exactly; one more; two segments and one, odd width; three segments
FRAMES = [(1, 1), (S + 1, 1), (1, S + 1), (S, S), (S + 1, S + 1), (65, 2 * S + 1),
          (min(3 * S + 1, 200), 67)]
DISTS = sorted({min(v, 255) for v in (1, 2, S - 1, S, S + 1, 255)} - {0})
frame_id = lambda f: "%dx%d" % f


def same32(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def stack_of(W, H, seed=0, invalid=INVALID):
    """Six maps [6][H][W] and their f32 planes, read-only: random with 10 %, 50 %
    and 100 % holes, all valid, one valid pixel in a corner, one in the centre."""
    maps = [fe.random_map(W, H, 100 * W + H + seed, holes=h, invalid=invalid) for h in (0.1, 0.5)]
    maps.append(fe.random_map(W, H, 7, holes=1.1, invalid=invalid))
    maps.append(fe.random_map(W, H, 8, holes=0.0, invalid=invalid))
    for y, x in ((H - 1, 0), (H // 2, W // 2)):
        m = maps[2].copy()
        m[y, x] = 9
        maps.append(m)
    d = np.stack(maps)
    s = fe.subpix_of(d, seed)
    d.setflags(write=False)
    s.setflags(write=False)
    return d, s


@functools.lru_cache(maxsize=None)
def keys_of(W, H, max_dist, seed=0, invalid=INVALID):
    k = fe.candidates(stack_of(W, H, seed, invalid)[0], invalid, max_dist)
    k.setflags(write=False)
    return k


def dev16(a, dev, offset=0):
    flat = torch.zeros(a.size + offset, dtype=torch.int16, device=dev)
    flat[offset:] = torch.from_numpy(a.view(np.int16).ravel().copy()).to(dev)
    return flat[offset:]


def run_d(ctx, dev, d, s, max_dist, min_found=1, mode=fe.SECOND, invalid=INVALID, want_sub=True,
          want_found=True, in_place=False, offset=0):
    """(out, out_sub, n_found) of sva_fill_holes_d; absent outputs None."""
    n, H, W = d.shape
    td = dev16(d, dev, offset)
    ts = torch.from_numpy(s.copy()).to(dev) if s is not None else None
    want_sub = want_sub and s is not None
    out = td if in_place else torch.full((d.size + offset,), 0x5A5A, dtype=torch.int16,
                                         device=dev)[offset:]
    osub = None if not want_sub else ts if in_place else torch.full(d.shape, 7.0, device=dev)
    found = torch.full(d.shape, 0x6B, dtype=torch.uint8, device=dev) if want_found else None
    ptr = lambda t: None if t is None else t.data_ptr()
    ctx.fill_holes_d(ptr(td), ptr(ts), n, W, H, invalid, max_dist, min_found, mode, ptr(out),
                     ptr(osub), ptr(found))
    ctx.synchronize()
    torch.cuda.synchronize()
    return (out.cpu().numpy().view(np.uint16).reshape(d.shape),
            None if osub is None else osub.cpu().numpy().reshape(d.shape),
            None if found is None else found.cpu().numpy())


def check(got, d, s, keys, min_found, mode, invalid=INVALID):
    out, osub, found = got
    eo, es, ef, filled = fe.apply(d, keys, invalid, min_found, mode, s)
    assert np.array_equal(out, eo), int((out != eo).sum())
    if osub is not None:
        assert same32(osub, es), int((osub.view(np.uint32) != es.view(np.uint32)).sum())
    if found is not None:
        assert np.array_equal(found, ef), int((found != ef).sum())
    return filled


@pytest.mark.parametrize("frame", FRAMES, ids=frame_id)
@pytest.mark.parametrize("max_dist", DISTS)
def test_maps_modes_and_counts(ctx, torch_dev, max_dist, frame):
    """All three modes x min_found in {1, 3, 8} on the six maps."""
    W, H = frame
    d, s = stack_of(W, H)
    keys = keys_of(W, H, max_dist)
    for mode in fe.MODES:
        for mf in (1, 3, 8):
            filled = check(run_d(ctx, torch_dev, d, s, max_dist, mf, mode), d, s, keys, mf, mode)
            assert not filled[3].any()                       # the all-valid map
            if mf > 1:
                assert not filled[4].any()                   # one source: one candidate at most


def test_the_cases_reach_every_outcome():
    """What the maps must contain for the comparisons to mean something."""
    W, H = FRAMES[-1]
    d, s = stack_of(W, H)
    keys = keys_of(W, H, S + 1)
    hole = ~fe.valid(d, INVALID)
    assert hole[2].all() and not hole[3].any() and hole[4].sum() == W * H - 1
    assert (d == 0).any() and (d == INVALID).any()
    n = (keys != fe.ABSENT).sum(axis=0)
    n_near = (keys_of(W, H, 2) != fe.ABSENT).sum(axis=0)
    assert set(n[hole].ravel().tolist()) | set(n_near[hole].ravel().tolist()) == set(range(9))
    picks = [fe.apply(d, keys, INVALID, 1, mode, s)[0] for mode in fe.MODES]
    assert not np.array_equal(picks[0], picks[1]) and not np.array_equal(picks[1], picks[2])
    assert ((keys >> 3 & 255)[keys != fe.ABSENT] > S).any()   # a source beyond one segment
    for mf in (3, 8):
        filled = fe.apply(d, keys, INVALID, mf, fe.MEDIAN)[3]
        assert filled.any() and (hole & ~filled & (n > 0)).any()


@pytest.mark.parametrize("corner", ["first", "last"])
@pytest.mark.parametrize("frame", [(257, 1), (1, 257), (257, 257)], ids=frame_id)
def test_distance_limit(ctx, torch_dev, frame, corner):
    """One valid pixel in a corner, max_dist 255: the hole 255 steps away along
    the row, the column and the diagonal is filled, the one 256 away is not."""
    W, H = frame
    d = np.zeros((1, H, W), np.uint16)
    y0, x0 = (0, 0) if corner == "first" else (H - 1, W - 1)
    d[0, y0, x0] = 77
    s = np.arange(W * H, dtype=np.float32).reshape(1, H, W)
    out, osub, found = run_d(ctx, torch_dev, d, s, 255)
    sign = 1 if corner == "first" else -1
    at = lambda j, ux, uy: (0, y0 + sign * j * uy, x0 + sign * j * ux)
    lines = [(1, 0)] * (W > 1) + [(0, 1)] * (H > 1) + [(1, 1)] * (W > 1 and H > 1)
    for ux, uy in lines:
        near, far, one = at(255, ux, uy), at(256, ux, uy), at(1, ux, uy)
        assert out[near] == 77 and found[near] == 1 and osub[near] == s[0, y0, x0]
        assert out[one] == 77 and found[one] == 1
        assert out[far] == 0 and found[far] == 0 and osub[far] == s[far]
    assert (out == 77).sum() == 1 + 255 * len(lines)
    check((out, osub, found), d, s, fe.candidates(d, INVALID, 255), 1, fe.SECOND)


def test_tie_breaks(ctx, torch_dev):
    """Equal d at different j: the nearer wins.  Equal (d, j) in two directions:
    the lower k wins, and out_sub shows which source that was."""
    d = np.zeros((2, 7, 7), np.uint16)
    s = np.arange(2 * 49, dtype=np.float32).reshape(2, 7, 7) + 0.25
    # map 0, hole (3, 3): 5 at E j = 2 and W j = 1 and N j = 3 -> sorted W, E, N
    d[0, 3, 5], d[0, 3, 2], d[0, 0, 3] = 5, 5, 5
    d[0, 3, 6] = 1                      # behind the E source: never seen from (3, 3)
    # map 1, hole (3, 3): 5 at j = 2 in E (k 0), S (k 2) and NW (k 5), 9 at W j = 1
    d[1, 3, 5], d[1, 5, 3], d[1, 1, 1], d[1, 3, 2] = 5, 5, 5, 9
    want = {fe.MIN: ((3, 2), (3, 5)), fe.SECOND: ((3, 5), (5, 3)), fe.MEDIAN: ((3, 5), (5, 3))}
    for mode in fe.MODES:
        out, osub, found = run_d(ctx, torch_dev, d, s, 4, 1, mode)
        check((out, osub, found), d, s, fe.candidates(d, INVALID, 4), 1, mode)
        assert found[0, 3, 3] == 3 and found[1, 3, 3] == 4
        for m in (0, 1):
            assert out[m, 3, 3] == 5 and osub[m, 3, 3] == s[(m,) + want[mode][m]], (mode, m)


def test_maps_do_not_interact(ctx, torch_dev):
    """Map k is map 0 rolled and raised: a value leaking between maps shows."""
    W, H = S + 1, S + 1
    d0 = fe.random_map(W, H, 5, holes=0.5)
    maps = []
    for k in range(3):
        m = np.roll(d0, (k, 2 * k), axis=(0, 1)).copy()
        keep = fe.valid(m, INVALID)
        m[keep] += 50 * k
        maps.append(m)
    d = np.stack(maps)
    s = fe.subpix_of(d, 1)
    keys = fe.candidates(d, INVALID, 6)
    got = run_d(ctx, torch_dev, d, s, 6, 2, fe.MEDIAN)
    check(got, d, s, keys, 2, fe.MEDIAN)
    for k in range(3):
        alone = run_d(ctx, torch_dev, d[k:k + 1], s[k:k + 1], 6, 2, fe.MEDIAN)
        assert np.array_equal(alone[0][0], got[0][k]) and same32(alone[1][0], got[1][k])
        ok = fe.valid(got[0][k], INVALID)
        assert (got[0][k][ok] > 50 * k).all() and (got[0][k][ok] <= 50 * k + 40).all()


@pytest.mark.parametrize("max_dist", [0, S + 1])
@pytest.mark.parametrize("want_sub,want_found,with_sub", [
    (True, True, True), (True, False, True), (False, True, True), (False, False, True),
    (False, True, False), (False, False, False)])
def test_absent_outputs(ctx, torch_dev, want_sub, want_found, with_sub, max_dist):
    """Every combination of the optional planes, also at max_dist 0 (the copy,
    which takes no workspace)."""
    W, H = FRAMES[4]
    d, s = stack_of(W, H)
    got = run_d(ctx, torch_dev, d, s if with_sub else None, max_dist, 2, fe.MEDIAN,
                want_sub=want_sub, want_found=want_found)
    assert (got[1] is not None) == (want_sub and with_sub) and (got[2] is not None) == want_found
    filled = check(got, d, s if with_sub else None, keys_of(W, H, max_dist), 2, fe.MEDIAN)
    if max_dist == 0:
        assert not filled.any() and np.array_equal(got[0], d)
        assert got[1] is None or same32(got[1], s)
        assert got[2] is None or not got[2].any()


@pytest.mark.parametrize("frame", [FRAMES[4], FRAMES[-1], (1, 1)], ids=frame_id)
@pytest.mark.parametrize("max_dist", [0, 5, 255])
def test_in_place(ctx, torch_dev, frame, max_dist):
    """out == disps and out_sub == subpix, with and without n_found."""
    W, H = frame
    d, s = stack_of(W, H)
    keys = keys_of(W, H, max_dist)
    for want_found in (True, False):
        check(run_d(ctx, torch_dev, d, s, max_dist, 1, fe.SECOND, in_place=True,
                    want_found=want_found), d, s, keys, 1, fe.SECOND)


@pytest.mark.parametrize("frame", [FRAMES[4], (3, 5), (1, 1)], ids=frame_id)
def test_two_byte_aligned_views(ctx, torch_dev, frame):
    """The u16 planes one element into a larger tensor: the base is 2-byte
    aligned only, and at odd W so is every other row; also in place."""
    W, H = frame
    d, s = stack_of(W, H)
    keys = keys_of(W, H, 5)
    check(run_d(ctx, torch_dev, d, s, 5, 2, fe.MEDIAN, offset=1), d, s, keys, 2, fe.MEDIAN)
    check(run_d(ctx, torch_dev, d, s, 5, 2, fe.MEDIAN, offset=1, in_place=True), d, s, keys, 2,
          fe.MEDIAN)


def test_workspace_reuse_and_regrowth(ctx, torch_dev):
    """A large frame, smaller ones in the kept workspace (whose planes hold the
    first call's keys), then the large one again."""
    for W, H in (FRAMES[-1], FRAMES[3], (7, 3), FRAMES[-1]):
        d, s = stack_of(W, H)
        check(run_d(ctx, torch_dev, d, s, 9, 3, fe.MEDIAN), d, s, keys_of(W, H, 9), 3, fe.MEDIAN)


def test_another_invalid(ctx, torch_dev):
    """An `invalid` that is not 0xFFFF: 0xFFFF is then a disparity like any
    other, and a large one (the key's top bits)."""
    W, H = FRAMES[4]
    d = stack_of(W, H, 3, 77)[0].copy()
    d[:, ::5, ::3] = 0xFFFF
    d[:, 1::5, ::3] = 0xFFFE
    s = fe.subpix_of(d, 2)
    keys = fe.candidates(d, 77, 6)
    for mode in fe.MODES:
        got = run_d(ctx, torch_dev, d, s, 6, 1, mode, invalid=77)
        check(got, d, s, keys, 1, mode, invalid=77)
    assert (got[0][~fe.valid(d, 77)] >= 0xFFFE).any()


@pytest.mark.parametrize("frame", [(1, 1), FRAMES[4], FRAMES[-1]], ids=frame_id)
def test_host_twin_equals_device_entry(ctx, sva, torch_dev, frame):
    W, H = frame
    d, s = stack_of(W, H)
    dev = run_d(ctx, torch_dev, d, s, 9, 2, fe.SECOND)
    check(dev, d, s, keys_of(W, H, 9), 2, fe.SECOND)
    ctx.set_timing(sva.SVA_TIMING_ALL)
    ctx.reset_timing()
    try:
        host = ctx.fill_holes(d, 9, 2, sva.SVA_FILL_SECOND, s)
        assert ctx.kernel_time("fill_scan")[1] == 1 and ctx.kernel_time("fill_apply")[1] == 1
        copy = ctx.fill_holes(d, 0, 2, sva.SVA_FILL_SECOND, s, want_found=False)
        assert ctx.kernel_time("fill_scan")[1] == 1 and ctx.kernel_time("fill_apply")[1] == 2
    finally:
        ctx.set_timing(0)
    assert np.array_equal(host[0], dev[0]) and same32(host[1], dev[1])
    assert np.array_equal(host[2], dev[2])
    assert np.array_equal(copy[0], d) and same32(copy[1], s) and copy[2] is None
    bare = ctx.fill_holes(d, 9, 2, sva.SVA_FILL_SECOND, None, want_found=False)
    assert np.array_equal(bare[0], dev[0]) and bare[1] is None and bare[2] is None
    # the host entry in place
    d2, s2 = d.copy(), s.copy()
    st = sva.lib.sva_fill_holes(ctx.h, d2.ctypes.data, s2.ctypes.data, d.shape[0], W, H, INVALID, 9,
                                2, sva.SVA_FILL_SECOND, d2.ctypes.data, s2.ctypes.data, None)
    assert st == 0 and np.array_equal(d2, dev[0]) and same32(s2, dev[1])
    assert (sva.SVA_FILL_MIN, sva.SVA_FILL_SECOND, sva.SVA_FILL_MEDIAN) == fe.MODES


def test_segment_length_does_not_change_the_result(ctx, sva, torch_dev):
    """SVA_DEBUG_FILL_SEGMENT is speed only."""
    W, H = FRAMES[-1]
    d, s = stack_of(W, H)
    assert ctx.get_debug(sva.SVA_DEBUG_FILL_SEGMENT) == S
    try:
        for seg in (1, 7, 64, 4096):
            ctx.set_debug(sva.SVA_DEBUG_FILL_SEGMENT, seg)
            assert ctx.get_debug(sva.SVA_DEBUG_FILL_SEGMENT) == seg
            check(run_d(ctx, torch_dev, d, s, 9, 2, fe.MEDIAN), d, s, keys_of(W, H, 9), 2, fe.MEDIAN)
    finally:
        ctx.set_debug(sva.SVA_DEBUG_FILL_SEGMENT, 0)
    assert ctx.get_debug(sva.SVA_DEBUG_FILL_SEGMENT) == S


def test_argument_errors_write_nothing(ctx, sva, torch_dev):
    """Every refusal of both entries, in the stated order: the status,
    canary-filled outputs untouched and no kernel launched."""
    W, H = FRAMES[4]
    d, s = stack_of(W, H)
    d, s = d[:2], s[:2]
    n = 2
    INV, UNS, OOM = sva.SVA_ERR_INVALID_ARG, sva.SVA_ERR_UNSUPPORTED, sva.SVA_ERR_OUT_OF_MEMORY
    np_ = n * W * H

    def host_buffers():
        b = dict(d=np.zeros(2 * np_, np.uint16), s=np.zeros(2 * np_, np.float32),
                 found=np.full(2 * np_, 0x6B, np.uint8))
        b["d"][:np_], b["d"][np_:] = d.ravel(), 0x5A5A
        b["s"][:np_], b["s"][np_:] = s.ravel(), 7.0
        return b

    def dev_buffers():
        return {k: torch.from_numpy(v.view({1: np.uint8, 2: np.int16, 4: np.int32}[v.itemsize]).copy())
                .to(torch_dev) for k, v in host_buffers().items()}

    def base_of(b, host):
        return {k: (v.ctypes.data if host else v.data_ptr()) for k, v in b.items()}

    # (plane, byte offset) names a pointer; the inputs lead their allocations,
    # the outputs follow them
    OUT, OSUB, FOUND = ("d", 2 * np_), ("s", 4 * np_), ("found", 0)
    cases = [
        ("null_disps", INV, "null pointer", dict(d=None)),
        ("null_out", INV, "null pointer", dict(out=None)),
        ("n_0", INV, "n_maps", dict(n=0)), ("n_negative", INV, "n_maps", dict(n=-1)),
        ("zero_width", INV, "image size", dict(W=0)),
        ("negative_height", INV, "image size", dict(H=-1)),
        ("too_many_pixels", UNS, "2^31", dict(W=65536, H=32768)),
        ("max_dist_negative", INV, "max_dist", dict(md=-1)),
        ("max_dist_256", INV, "max_dist", dict(md=256)),
        ("min_found_0", INV, "min_found", dict(mf=0)),
        ("min_found_9", INV, "min_found", dict(mf=9)),
        ("mode_negative", INV, "mode", dict(mode=-1)), ("mode_3", INV, "mode", dict(mode=3)),
        ("out_sub_without_subpix", INV, "out_sub needs subpix", dict(s=None)),
        ("out_in_disps", INV, "overlaps", dict(out=("d", 2))),
        ("out_before_disps_end", INV, "overlaps", dict(out=("d", 2 * np_ - 2))),
        ("out_in_subpix", INV, "overlaps", dict(out=("s", 0))),
        ("out_in_out_sub", INV, "overlaps", dict(out=("s", 4 * np_ + 4))),
        ("out_in_n_found", INV, "overlaps", dict(out=("found", 8))),
        ("out_sub_in_disps", INV, "overlaps", dict(osub=("d", 0))),
        ("out_sub_in_subpix", INV, "overlaps", dict(osub=("s", 4))),
        ("out_sub_is_n_found", INV, "overlaps", dict(osub=("found", 0))),
        ("n_found_in_disps", INV, "overlaps", dict(found=("d", 0))),
        ("n_found_is_subpix", INV, "overlaps", dict(found=("s", 0))),
        ("n_found_in_out", INV, "overlaps", dict(found=("d", 2 * np_))),
        # the order: each of these breaks the rule named first and later ones too
        ("null_before_size", INV, "null pointer", dict(d=None, W=0, md=-1)),
        ("n_before_size", INV, "n_maps", dict(n=0, H=0)),
        ("size_before_unsupported", INV, "image size", dict(W=-1, H=2 ** 31 - 1, md=999)),
        ("unsupported_before_max_dist", UNS, "2^31", dict(W=65536, H=32768, md=256)),
        ("max_dist_before_min_found", INV, "max_dist", dict(md=256, mf=0, mode=3)),
        ("min_found_before_mode", INV, "min_found", dict(mf=9, mode=3, s=None)),
        ("mode_before_out_sub", INV, "mode", dict(mode=3, s=None)),
        ("out_sub_before_overlap", INV, "out_sub needs subpix", dict(s=None, out=("d", 2))),
    ]
    ctx.set_timing(sva.SVA_TIMING_ALL)
    ctx.reset_timing()
    try:
        for host in (True, False):
            fn = sva.lib.sva_fill_holes if host else sva.lib.sva_fill_holes_d
            todo = list(cases)
            if not host:
                # 32 * n * W * H = 2^55 bytes of workspace, in place so that nothing overlaps
                todo.append(("workspace", OOM, "fill workspace",
                             dict(n=2 ** 30, W=1024, H=1024, out=("d", 0), osub=None, found=None,
                                  s=None)))
            for name, status, text, ch in todo:
                b = host_buffers() if host else dev_buffers()
                base = base_of(b, host)
                at = lambda v: None if v is None else base[v[0]] + v[1]
                a = dict(d=("d", 0), s=("s", 0), out=OUT, osub=OSUB, found=FOUND, n=n, W=W, H=H,
                         md=5, mf=1, mode=1)
                a.update(ch)
                st = fn(ctx.h, at(a["d"]), at(a["s"]), a["n"], a["W"], a["H"], INVALID, a["md"],
                        a["mf"], a["mode"], at(a["out"]), at(a["osub"]), at(a["found"]))
                msg = sva.lib.sva_last_error(ctx.h).decode()
                assert st == status and text in msg, (name, host, st, msg)
                ctx.synchronize()
                torch.cuda.synchronize()
                now = b if host else {k: v.cpu().numpy() for k, v in b.items()}
                ref = host_buffers()
                for k in ref:
                    assert np.array_equal(now[k].view(np.uint8), ref[k].view(np.uint8)), (name, k)
        for name in ("fill_scan", "fill_apply"):
            assert ctx.kernel_time(name)[1] == 0, name
    finally:
        ctx.set_timing(0)
    # the context still works, and a failed allocation left no error behind
    check(run_d(ctx, torch_dev, d, s, 5, 1, fe.SECOND), d, s, fe.candidates(d, INVALID, 5), 1,
          fe.SECOND)
