"""sva_filter_speckles / sva_filter_speckles_d on the
GPU: every output byte for byte against tests/speckle_expect.py, at the frame
sizes around the label pass's tile where the kernels can go wrong, on random
maps and on the shapes that stress the merge (snake, spiral, checkerboard, one
component, a ring); in place; 2-byte aligned views; workspace reuse; the host
twin; the refusals with nothing written."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import speckle_expect as se

pytestmark = pytest.mark.gpu

INVALID = 0xFFFF
_TUNING = os.path.join(os.path.dirname(__file__), "..", "stereovisionarray_amd", "csrc",
                       "sva_tuning.h")
TW, TH = map(int, re.search(r"kSpeckleTileW = (\d+), kSpeckleTileH = (\d+)",
                            open(_TUNING).read()).groups())
# (W, H): one pixel; one row and one column a pixel longer than the tile; the
# tile exactly (and transposed); one more each way; 3 x 3 tiles and one more
FRAMES = [(1, 1), (TW + 1, 1), (1, TH + 1), (TW, TH), (TH, TW), (TW + 1, TH + 1),
          (min(3 * TW + 1, 200), min(3 * TH + 1, 100))]
SHAPES = dict(snake=se.snake, spiral=se.spiral, checkerboard=se.checkerboard, solid=se.solid,
              ring=se.u_shape)
frame_id = lambda f: "%dx%d" % f


def same32(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def subpix_of(d, seed=0):
    """f32 planes with fractions and a few NaN of their own."""
    rng = np.random.default_rng(seed)
    s = (d.astype(np.float32) + rng.random(d.shape, dtype=np.float32) - 0.5).astype(np.float32)
    s[rng.random(d.shape) < 0.03] = np.nan
    return s


@functools.lru_cache(maxsize=None)
def stack_of(W, H, n, seed=0, hi=None, invalid=INVALID):
    """n maps: map 0 random, map k map 0 rolled by (k, 2k) with its values raised
    by k % 3 -- so a label leaking between maps shows; and their f32 planes.
    Read-only."""
    d0 = se.random_map(W, H, 100 * W + H + seed, invalid=invalid, hi=hi)
    maps = []
    for k in range(n):
        m = np.roll(d0, (k, 2 * k), axis=(0, 1)).copy()
        keep = se.valid(m, invalid)
        m[keep] = np.minimum(m[keep].astype(np.int64) + k % 3, 65534).astype(np.uint16)
        maps.append(m)
    d = np.stack(maps)
    s = subpix_of(d, seed)
    d.setflags(write=False)
    s.setflags(write=False)
    return d, s


@functools.lru_cache(maxsize=None)
def sizes_of(key, invalid, max_diff):
    """comp_size of a cached stack (key: stack_of's arguments) or shape ((name, W, H))."""
    d = SHAPES[key[0]](key[1], key[2])[None] if isinstance(key[0], str) else stack_of(*key)[0]
    size = se.comp_size(d, invalid, max_diff)
    size.setflags(write=False)
    return size


def dev16(a, dev, offset=0):
    flat = torch.zeros(a.size + offset, dtype=torch.int16, device=dev)
    flat[offset:] = torch.from_numpy(a.view(np.int16).ravel().copy()).to(dev)
    return flat[offset:]


def run_d(ctx, dev, d, s, max_size, max_diff, invalid=INVALID, want_sub=True, want_size=True,
          in_place=False, offset=0):
    """(out, out_sub, comp_size) of sva_filter_speckles_d; absent outputs None."""
    n, H, W = d.shape
    td = dev16(d, dev, offset)
    ts = torch.from_numpy(s.copy()).to(dev) if s is not None else None
    want_sub = want_sub and s is not None
    out = td if in_place else torch.full((d.size + offset,), 0x5A5A, dtype=torch.int16,
                                         device=dev)[offset:]
    osub = None if not want_sub else ts if in_place else torch.full(d.shape, 7.0, device=dev)
    size = torch.full(d.shape, 0x6B6B6B6B, dtype=torch.int32, device=dev) if want_size else None
    ptr = lambda t: None if t is None else t.data_ptr()
    ctx.filter_speckles_d(ptr(td), ptr(ts), n, W, H, invalid, max_size, max_diff, ptr(out),
                          ptr(osub), ptr(size))
    ctx.synchronize()
    torch.cuda.synchronize()
    return (out.cpu().numpy().view(np.uint16).reshape(d.shape),
            None if osub is None else osub.cpu().numpy().reshape(d.shape),
            None if size is None else size.cpu().numpy().view(np.uint32))


def check(got, d, s, size, max_size, invalid=INVALID):
    out, osub, gsize = got
    eo, es, gone = se.apply(d, size, invalid, max_size, s)
    assert np.array_equal(out, eo), int((out != eo).sum())
    if osub is not None:
        assert same32(osub, es), int((osub.view(np.uint32) != es.view(np.uint32)).sum())
        assert same32(osub[~gone], s[~gone]) and np.isnan(osub[gone]).all()
    if gsize is not None:
        assert np.array_equal(gsize, size), int((gsize != size).sum())
    return gone


@pytest.mark.parametrize("frame", FRAMES, ids=frame_id)
@pytest.mark.parametrize("n", [1, 2, 9, 33])
def test_random_maps(ctx, torch_dev, n, frame):
    """max_diff in {0, 1, 3, 65535} x max_size in {0, 1, 5, W*H - 1, W*H}."""
    W, H = frame
    d, s = stack_of(W, H, n)
    for md in (0, 1, 3, 65535):
        size = sizes_of((W, H, n), INVALID, md)
        for ms in sorted({0, 1, 5, W * H - 1, W * H}):
            gone = check(run_d(ctx, torch_dev, d, s, ms, md), d, s, size, ms)
            if ms == 0:
                assert not gone.any()
            if ms == W * H:
                assert gone.sum() == se.valid(d, INVALID).sum()


def test_the_cases_reach_every_outcome():
    """What the random maps must contain for the comparisons to mean something:
    components of one pixel, of a few, and one that spans tiles; removed and kept
    pixels at one threshold; maps that differ."""
    W, H = FRAMES[-1]
    d, _ = stack_of(W, H, 5)
    s0, s1 = sizes_of((W, H, 5), INVALID, 0), sizes_of((W, H, 5), INVALID, 1)
    assert (s0 == 1).any() and ((s0 > 1) & (s0 <= 5)).any() and (s0 != s1).any()
    assert s1.max() > TW * TH and (s1 == 0).any()
    assert (d == 0).any() and (d == INVALID).any()
    assert not np.array_equal(s1[0], s1[1])


@pytest.mark.parametrize("frame", FRAMES, ids=frame_id)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_shapes(ctx, torch_dev, shape, frame):
    """Long thin components across every tile border, every pixel its own
    component, one component; thresholds just below and at the component size."""
    W, H = frame
    d = SHAPES[shape](W, H)[None]
    s = d.astype(np.float32)
    for md in (0, 2):
        size = sizes_of((shape, W, H), INVALID, md)
        big = int(size.max())
        for ms in sorted({1, max(big - 1, 0), big}):
            check(run_d(ctx, torch_dev, d, s, ms, md), d, s, size, ms)
    if shape == "checkerboard":
        assert (sizes_of((shape, W, H), INVALID, 0) == 1).all()
    if shape in ("snake", "solid", "ring"):
        assert len(set(sizes_of((shape, W, H), INVALID, 0).ravel().tolist()) - {0}) == 1


@pytest.mark.parametrize("invalid", [INVALID, 77])
def test_large_disparities_and_another_invalid(ctx, torch_dev, invalid):
    """Values up to 65534 next to small ones (differences up to 65524), and an
    `invalid` that is not 0xFFFF: 0xFFFF is then a disparity like any other."""
    W, H = TW + 1, TH + 1
    d, s = stack_of(W, H, 2, 3, 65534, invalid)
    if invalid != INVALID:
        d = d.copy()
        d[0, 0, :3] = 0xFFFF
        d[0, 1, :3] = 0xFFFE
    assert d.max() >= 65534 and (d == invalid).any()
    for md in (1, 65535):
        size = se.comp_size(d, invalid, md)
        for ms in (1, 5):
            check(run_d(ctx, torch_dev, d, s, ms, md, invalid), d, s, size, ms, invalid)
    # max_diff above 65535 is 65535
    check(run_d(ctx, torch_dev, d, s, 5, 2 ** 31 - 1, invalid), d, s, size, 5, invalid)
    check(run_d(ctx, torch_dev, d, s, 2 ** 31 - 1, 1, invalid), d, s,
          se.comp_size(d, invalid, 1), 2 ** 31 - 1, invalid)


@pytest.mark.parametrize("ms", [0, 5])
@pytest.mark.parametrize("want_sub,want_size,with_sub", [
    (True, True, True), (True, False, True), (False, True, True), (False, False, True),
    (False, True, False), (False, False, False)])
def test_absent_outputs(ctx, torch_dev, want_sub, want_size, with_sub, ms):
    """Every combination of the optional planes, also at max_size 0 (with no
    comp_size: the copy, which takes no workspace)."""
    W, H = TW + 1, TH + 1
    d, s = stack_of(W, H, 2)
    got = run_d(ctx, torch_dev, d, s if with_sub else None, ms, 1, want_sub=want_sub,
                want_size=want_size)
    assert (got[1] is not None) == (want_sub and with_sub) and (got[2] is not None) == want_size
    check(got, d, s if with_sub else None, sizes_of((W, H, 2), INVALID, 1), ms)


@pytest.mark.parametrize("frame", [(TW + 1, TH + 1), FRAMES[-1], (1, 1)], ids=frame_id)
@pytest.mark.parametrize("ms", [0, 5])
def test_in_place(ctx, torch_dev, frame, ms):
    """out == disps and out_sub == subpix, with and without comp_size."""
    W, H = frame
    d, s = stack_of(W, H, 2)
    size = sizes_of((W, H, 2), INVALID, 1)
    for want_size in (True, False):
        check(run_d(ctx, torch_dev, d, s, ms, 1, in_place=True, want_size=want_size), d, s, size, ms)


@pytest.mark.parametrize("frame", [(TW + 1, TH + 1), (3, 5), (1, 1)], ids=frame_id)
def test_two_byte_aligned_views(ctx, torch_dev, frame):
    """The u16 planes one element into a larger tensor: the base is 2-byte
    aligned only, and at odd W so is every other row; also in place."""
    W, H = frame
    d, s = stack_of(W, H, 2)
    size = sizes_of((W, H, 2), INVALID, 1)
    check(run_d(ctx, torch_dev, d, s, 5, 1, offset=1), d, s, size, 5)
    check(run_d(ctx, torch_dev, d, s, 5, 1, offset=1, in_place=True), d, s, size, 5)


def test_workspace_reuse_and_regrowth(ctx, torch_dev):
    """A large frame, a smaller one in the kept workspace (whose planes hold the
    first call's labels), then one larger than both."""
    for W, H, n in ((TW + 1, TH + 1, 9), (TH, TW, 2), (7, 3, 1), FRAMES[-1] + (5,)):
        d, s = stack_of(W, H, n)
        check(run_d(ctx, torch_dev, d, s, 5, 1), d, s, sizes_of((W, H, n), INVALID, 1), 5)


@pytest.mark.parametrize("n,frame", [(1, (1, 1)), (2, (TW + 1, TH + 1)), (5, FRAMES[-1])])
def test_host_twin_equals_device_entry(ctx, sva, torch_dev, n, frame):
    W, H = frame
    d, s = stack_of(W, H, n)
    dev = run_d(ctx, torch_dev, d, s, 5, 1)
    check(dev, d, s, sizes_of((W, H, n), INVALID, 1), 5)
    ctx.set_timing(sva.SVA_TIMING_ALL)
    ctx.reset_timing()
    try:
        host = ctx.filter_speckles(d, 5, 1, s)
        for name in ("speckle_label", "speckle_merge", "speckle_count", "speckle_apply"):
            assert ctx.kernel_time(name)[1] == 1, name
        copy = ctx.filter_speckles(d, 0, 1, s, want_size=False)
        assert ctx.kernel_time("speckle_label")[1] == 1 and ctx.kernel_time("speckle_apply")[1] == 2
    finally:
        ctx.set_timing(0)
    assert np.array_equal(host[0], dev[0]) and same32(host[1], dev[1])
    assert np.array_equal(host[2], dev[2])
    assert np.array_equal(copy[0], d) and same32(copy[1], s) and copy[2] is None
    bare = ctx.filter_speckles(d, 5, 1, None, want_size=False)
    assert np.array_equal(bare[0], dev[0]) and bare[1] is None and bare[2] is None
    # the host entry in place
    d2, s2 = d.copy(), s.copy()
    st = sva.lib.sva_filter_speckles(ctx.h, d2.ctypes.data, s2.ctypes.data, n, W, H, INVALID, 5, 1,
                                     d2.ctypes.data, s2.ctypes.data, None)
    assert st == 0 and np.array_equal(d2, dev[0]) and same32(s2, dev[1])


def test_argument_errors_write_nothing(ctx, sva, torch_dev):
    """Every refusal of both entries: the status, canary-filled outputs
    untouched and no kernel launched."""
    n, W, H = 2, TW + 1, TH + 1
    d, s = stack_of(W, H, n)
    INV, UNS, OOM = sva.SVA_ERR_INVALID_ARG, sva.SVA_ERR_UNSUPPORTED, sva.SVA_ERR_OUT_OF_MEMORY
    np_ = n * W * H

    def host_buffers():
        b = dict(d=np.zeros(2 * np_, np.uint16), s=np.zeros(2 * np_, np.float32),
                 size=np.full(2 * np_, 0x6B6B6B6B, np.uint32))
        b["d"][:np_], b["d"][np_:] = d.ravel(), 0x5A5A
        b["s"][:np_], b["s"][np_:] = s.ravel(), 7.0
        return b

    def dev_buffers():
        return {k: torch.from_numpy(v.view({2: np.int16, 4: np.int32}[v.itemsize]).copy())
                .to(torch_dev) for k, v in host_buffers().items()}

    def base_of(b, host):
        return {k: (v.ctypes.data if host else v.data_ptr()) for k, v in b.items()}

    # (plane, byte offset) names a pointer; the inputs lead their allocations,
    # the outputs follow them: d+2np_ etc.
    OUT, OSUB, SIZE = ("d", 2 * np_), ("s", 4 * np_), ("size", 0)
    cases = [
        ("n_0", INV, dict(n=0)), ("n_negative", INV, dict(n=-1)),
        ("null_disps", INV, dict(d=None)), ("null_out", INV, dict(out=None)),
        ("zero_width", INV, dict(W=0)), ("negative_height", INV, dict(H=-1)),
        ("max_size_negative", INV, dict(ms=-1)), ("max_diff_negative", INV, dict(md=-1)),
        ("out_sub_without_subpix", INV, dict(s=None)),
        ("out_in_disps", INV, dict(out=("d", 2))),
        ("out_before_disps_end", INV, dict(out=("d", 2 * np_ - 2))),
        ("out_in_subpix", INV, dict(out=("s", 0))),
        ("out_in_out_sub", INV, dict(out=("s", 4 * np_ + 4))),
        ("out_in_comp_size", INV, dict(out=("size", 8))),
        ("out_sub_in_disps", INV, dict(osub=("d", 0))),
        ("out_sub_in_subpix", INV, dict(osub=("s", 4))),
        ("out_sub_is_comp_size", INV, dict(osub=("size", 0))),
        ("comp_size_in_disps", INV, dict(size=("d", 0))),
        ("comp_size_is_subpix", INV, dict(size=("s", 0))),
        ("comp_size_in_out", INV, dict(size=("d", 2 * np_))),
        ("too_many_pixels", UNS, dict(W=65536, H=32768)),
    ]
    ctx.set_timing(sva.SVA_TIMING_ALL)
    ctx.reset_timing()
    try:
        for host in (True, False):
            fn = sva.lib.sva_filter_speckles if host else sva.lib.sva_filter_speckles_d
            todo = list(cases)
            if not host:
                # 8 * n * W * H = 2^53 bytes of workspace, in place so that nothing overlaps
                todo.append(("workspace", OOM, dict(n=2 ** 30, W=1024, H=1024, out=("d", 0), osub=None,
                                                    size=None, s=None)))
            for name, status, ch in todo:
                b = host_buffers() if host else dev_buffers()
                base = base_of(b, host)
                at = lambda v: None if v is None else base[v[0]] + v[1]
                a = dict(d=("d", 0), s=("s", 0), out=OUT, osub=OSUB, size=SIZE, n=n, W=W, H=H, ms=5,
                         md=1)
                a.update(ch)
                st = fn(ctx.h, at(a["d"]), at(a["s"]), a["n"], a["W"], a["H"], INVALID, a["ms"],
                        a["md"], at(a["out"]), at(a["osub"]), at(a["size"]))
                assert st == status, (name, host, st, sva.lib.sva_last_error(ctx.h))
                ctx.synchronize()
                torch.cuda.synchronize()
                now = b if host else {k: v.cpu().numpy() for k, v in b.items()}
                ref = host_buffers()
                for k in ref:
                    assert np.array_equal(now[k].view(np.uint8), ref[k].view(np.uint8)), (name, k)
        for name in ("speckle_label", "speckle_merge", "speckle_count", "speckle_apply"):
            assert ctx.kernel_time(name)[1] == 0, name
    finally:
        ctx.set_timing(0)
    # the context still works, and a failed allocation left no error behind
    check(run_d(ctx, torch_dev, d, s, 5, 1), d, s, sizes_of((W, H, n), INVALID, 1), 5)
