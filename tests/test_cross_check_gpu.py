"""sva_cross_check / sva_cross_check_d on the GPU:
every output byte for byte against tests/cross_expect.py on random maps, at the
view counts, frame sizes, step sets and thresholds where the kernel can go
wrong; both block orders; the argument errors with nothing written."""
import functools

import numpy as np
import pytest
import torch

import cross_expect as ce

pytestmark = pytest.mark.gpu

INVALID = 0xFFFF
NS = [1, 2, 3, 9, 25, 32]
FRAMES = [(1, 1), (1, 37), (70, 1), (70, 37), (257, 5), (130, 66)]      # (W, H)
RIG3 = [(-gx, -gy) for gy in (-1, 0, 1) for gx in (-1, 0, 1)]
RIG5 = [(-gx, -gy) for gy in range(-2, 3) for gx in range(-2, 3)]
# no grid: negative components, +-255, steps two views apart by up to 510
LOOSE = [(0, 0), (-1, 2), (255, -255), (-255, 255), (3, 0), (0, -3), (-2, -2), (255, 0), (1, 1),
         (-255, -255), (2, -1), (-1, -1), (0, 5), (-4, 1), (1, -6), (7, 7), (-7, 3), (0, 255),
         (5, -2), (-3, -5), (6, 0), (0, -8), (-9, 9), (4, 4), (-1, 0), (0, 1), (8, -3), (-6, -6),
         (2, 3), (-5, 0), (10, 1), (1, -10)]
assert len(set(LOOSE)) == 32


def steps_of(n, kind):
    if kind == "rig":
        base = RIG3 if n <= 9 else RIG5 if n <= 25 else RIG5 + [(3, y) for y in range(-3, 4)]
        return base[:n]
    return LOOSE[:n]


@functools.lru_cache(maxsize=None)
def maps_of(n, W, H, seed=0, hi=40):
    """n random maps: values 0..hi (zeros among them), about 10 % INVALID; and
    f32 planes with fractions and a few NaN of their own.  Read-only."""
    rng = np.random.default_rng(1000 * n + 10 * W + H + seed)
    d = rng.integers(0, hi + 1, size=(n, H, W)).astype(np.uint16)
    d[rng.random((n, H, W)) < 0.1] = INVALID
    s = (d.astype(np.float32) + rng.random((n, H, W), dtype=np.float32) - 0.5).astype(np.float32)
    s[rng.random((n, H, W)) < 0.03] = np.nan
    d.setflags(write=False)
    s.setflags(write=False)
    return d, s


def same32(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def dev16(a, dev, offset=0):
    """A u16 array on the device, as an int16 tensor `offset` elements into a
    larger one (offset 1: a base that is only 2-byte aligned)."""
    flat = torch.zeros(a.size + offset, dtype=torch.int16, device=dev)
    flat[offset:] = torch.from_numpy(a.view(np.int16).ravel().copy()).to(dev)
    return flat[offset:]


def run_d(ctx, dev, d, s, steps, md, ma, mc, invalid=INVALID, want=(True, True, True), offset=0):
    """(out, out_sub, agree, conflict) of sva_cross_check_d; want: out_sub, agree,
    conflict.  Absent outputs come back None."""
    n, H, W = d.shape
    td = dev16(d, dev, offset)
    ts = torch.from_numpy(s.copy()).to(dev) if s is not None else None
    out = torch.full((d.size + offset,), 0x5A5A, dtype=torch.int16, device=dev)[offset:]
    osub = torch.full(d.shape, 7.0, dtype=torch.float32, device=dev) if want[0] else None
    ag = torch.full(d.shape, 0xEE, dtype=torch.uint8, device=dev) if want[1] else None
    cf = torch.full(d.shape, 0xEE, dtype=torch.uint8, device=dev) if want[2] else None
    ctx.cross_check_d(td.data_ptr(), ts.data_ptr() if ts is not None else None, n, W, H, steps,
                      invalid, md, ma, mc, out.data_ptr(),
                      osub.data_ptr() if osub is not None else None,
                      ag.data_ptr() if ag is not None else None,
                      cf.data_ptr() if cf is not None else None)
    ctx.synchronize()
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    return (out.cpu().numpy().view(np.uint16).reshape(d.shape), host(osub), host(ag), host(cf))


def check(got, d, s, agree, conflict, ma, mc, invalid=INVALID):
    out, osub, ag, cf = got
    eo, es, rej = ce.decide(d, agree, conflict, invalid, ma, mc, s)
    assert np.array_equal(out, eo), int((out != eo).sum())
    if osub is not None:
        assert same32(osub, es), int((osub.view(np.uint32) != es.view(np.uint32)).sum())
        # NaN exactly at the rejected pixels (and where the input had one), the input bits elsewhere
        assert np.array_equal(np.isnan(osub), rej | np.isnan(s))
        assert same32(osub[~rej], s[~rej])
    if ag is not None:
        assert np.array_equal(ag, agree.astype(np.uint8))
    if cf is not None:
        assert np.array_equal(cf, conflict.astype(np.uint8))
    return rej


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("n", NS)
def test_counts_and_decisions(ctx, torch_dev, n, frame):
    """Every (max_diff, min_agree, max_conflict) of {0, 1, 3} x {0, 1, n - 1} x
    {0, 31} on the rig steps and on the loose ones."""
    W, H = frame
    d, s = maps_of(n, W, H)
    for kind in ("rig", "loose"):
        steps = steps_of(n, kind)
        for md in (0, 1, 3):
            agree, conflict = ce.counts(d, steps, INVALID, md)
            for ma in sorted({0, 1, n - 1} - {-1, 32}):
                for mc in (0, 31):
                    got = run_d(ctx, torch_dev, d, s, steps, md, ma, mc)
                    rej = check(got, d, s, agree, conflict, ma, mc)
                    if ma == 0 and mc == 31:        # the identity
                        assert not rej.any() and np.array_equal(got[0], d) and same32(got[1], s)


def test_the_cases_reach_every_class():
    """What the random maps must contain for the comparisons above to mean
    something: agreeing, conflicting and occluded neighbours, targets outside."""
    d, _ = maps_of(9, 70, 37)
    agree, conflict = ce.counts(d, RIG3, INVALID, 1)
    a0, _ = ce.counts(d, RIG3, INVALID, 0)
    assert agree.max() >= 3 and conflict.max() >= 3 and (a0 != agree).any()
    assert (d == 0).any() and (d == INVALID).any()
    for ma, mc in ((1, 0), (2, 4), (0, 0)):
        rej = ce.decide(d, agree, conflict, INVALID, ma, mc)[2]
        assert rej.any() and (~rej & ce.valid(d, INVALID)).any()
    a25, c25 = ce.counts(maps_of(25, 130, 66)[0], RIG5, INVALID, 3)
    assert a25.max() > 8 and c25.max() > 8


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("n,frame", [(1, (70, 37)), (3, (257, 5)), (9, (130, 66)), (25, (130, 66)),
                                     (32, (70, 37)), (2, (1, 1))])
def test_both_block_orders(ctx, sva, torch_dev, order, n, frame):
    """The tile-major order's last group of 8 tiles is short at these sizes (34,
    6 and 11 tiles, or one); the order never changes a byte."""
    W, H = frame
    d, s = maps_of(n, W, H)
    steps = steps_of(n, "rig")
    agree, conflict = ce.counts(d, steps, INVALID, 1)
    ctx.set_debug(sva.SVA_DEBUG_CROSS_ORDER, order)
    try:
        assert ctx.get_debug(sva.SVA_DEBUG_CROSS_ORDER) == order
        got = run_d(ctx, torch_dev, d, s, steps, 1, 1, 0)
    finally:
        ctx.set_debug(sva.SVA_DEBUG_CROSS_ORDER, -1)
    check(got, d, s, agree, conflict, 1, 0)


def test_large_disparities_and_another_invalid(ctx, torch_dev):
    """Disparities up to 65534 next to small ones, along steps up to 510 apart:
    the products s * e reach 3.3e7; and an `invalid` that is not 0xFFFF."""
    n, W, H = 9, 130, 66
    rng = np.random.default_rng(9)
    d = rng.integers(0, 41, size=(n, H, W)).astype(np.uint16)
    big = rng.random((n, H, W)) < 0.3
    d[big] = rng.integers(60000, 65535, size=int(big.sum())).astype(np.uint16)
    d[0, 0, 0] = 65534
    d[rng.random((n, H, W)) < 0.1] = INVALID
    s = d.astype(np.float32)
    for steps in (RIG3, LOOSE[:n]):
        for invalid in (INVALID, 7):
            agree, conflict = ce.counts(d, steps, invalid, 3)
            assert conflict.any() and agree.any()
            check(run_d(ctx, torch_dev, d, s, steps, 3, 1, 0, invalid), d, s, agree, conflict, 1, 0,
                  invalid)


@pytest.mark.parametrize("want", [(False, True, True), (True, False, True), (True, True, False),
                                  (False, False, False)])
def test_absent_outputs(ctx, torch_dev, want):
    d, s = maps_of(9, 70, 37)
    agree, conflict = ce.counts(d, RIG3, INVALID, 1)
    check(run_d(ctx, torch_dev, d, s, RIG3, 1, 2, 1, want=want), d, s, agree, conflict, 2, 1)
    # no subpix at all
    got = run_d(ctx, torch_dev, d, None, RIG3, 1, 2, 1, want=(False, want[1], want[2]))
    check(got, d, None, agree, conflict, 2, 1)


@pytest.mark.parametrize("frame", [(37, 70), (257, 5), (1, 1)], ids=lambda f: "%dx%d" % f)
def test_two_byte_aligned_views(ctx, torch_dev, frame):
    """Input and output planes one u16 into a larger tensor: the base is 2-byte
    aligned only, and at odd W so is every other row."""
    W, H = frame
    d, s = maps_of(3, W, H)
    agree, conflict = ce.counts(d, RIG3[:3], INVALID, 1)
    check(run_d(ctx, torch_dev, d, s, RIG3[:3], 1, 1, 0, offset=1), d, s, agree, conflict, 1, 0)


@pytest.mark.parametrize("n,frame", [(1, (1, 1)), (9, (70, 37)), (32, (130, 66))])
def test_host_twin_equals_device_entry(ctx, sva, torch_dev, n, frame):
    W, H = frame
    d, s = maps_of(n, W, H)
    steps = steps_of(n, "loose")
    dev = run_d(ctx, torch_dev, d, s, steps, 1, 1, 1)
    ctx.set_timing(sva.SVA_TIMING_ALL)
    ctx.reset_timing()
    try:
        host = ctx.cross_check(d, steps, s, INVALID, 1, 1, 1)
        assert ctx.kernel_time("cross_check")[1] == 1
    finally:
        ctx.set_timing(0)
    assert np.array_equal(host[0], dev[0]) and same32(host[1], dev[1])
    assert np.array_equal(host[2], dev[2]) and np.array_equal(host[3], dev[3])
    bare = ctx.cross_check(d, steps, None, INVALID, 1, 1, 1, want_agree=False, want_conflict=False)
    assert np.array_equal(bare[0], dev[0]) and bare[1] is None and bare[2] is None and bare[3] is None


def test_argument_errors_write_nothing(ctx, sva, torch_dev):
    """Every refusal of both entries: the status, and canary-filled outputs
    untouched with no kernel launched."""
    n, W, H = 3, 70, 37
    d, s = maps_of(n, W, H)
    steps = RIG3[:n]
    INV, UNS = sva.SVA_ERR_INVALID_ARG, sva.SVA_ERR_UNSUPPORTED
    np_ = n * W * H

    def host_buffers():
        return dict(d=d.copy(), s=s.copy(), out=np.full(d.shape, 0x5A5A, np.uint16),
                    osub=np.full(d.shape, 7.0, np.float32), ag=np.full(d.shape, 0xEE, np.uint8),
                    cf=np.full(d.shape, 0xEE, np.uint8))

    def dev_buffers():
        # one allocation, so that overlapping ranges can be named
        flat = torch.zeros(np_ * 2 + 8, dtype=torch.int16, device=torch_dev)
        flat[:np_] = torch.from_numpy(d.view(np.int16).ravel().copy()).to(torch_dev)
        flat[np_:] = 0x5A5A
        fsub = torch.full((np_ * 2,), 7.0, dtype=torch.float32, device=torch_dev)
        fsub[:np_] = torch.from_numpy(s.ravel().copy()).to(torch_dev)
        cnt = torch.full((2 * np_,), 0xEE, dtype=torch.uint8, device=torch_dev)
        return dict(flat=flat, fsub=fsub, cnt=cnt)

    def ptrs_of(b, host):
        if host:
            return dict(d=b["d"].ctypes.data, s=b["s"].ctypes.data, out=b["out"].ctypes.data,
                        osub=b["osub"].ctypes.data, ag=b["ag"].ctypes.data, cf=b["cf"].ctypes.data)
        f, fs, c = b["flat"].data_ptr(), b["fsub"].data_ptr(), b["cnt"].data_ptr()
        return dict(d=f, s=fs, out=f + 2 * np_, osub=fs + 4 * np_, ag=c, cf=c + np_)

    dup = [(0, 0), (1, 0), (0, 0)]
    cases = [
        ("n_0", INV, dict(n=0)), ("n_33", INV, dict(n=33, steps=LOOSE + [(9, 9)])),
        ("null_disps", INV, dict(d=None)), ("null_view_step", INV, dict(steps=None)),
        ("null_out", INV, dict(out=None)),
        ("zero_width", INV, dict(W=0)), ("negative_height", INV, dict(H=-1)),
        ("step_256", INV, dict(steps=[(0, 0), (256, 0), (0, 1)])),
        ("step_minus_256", INV, dict(steps=[(0, 0), (1, 0), (0, -256)])),
        ("equal_steps", INV, dict(steps=dup)),
        ("max_diff_negative", INV, dict(md=-1)),
        ("min_agree_32", INV, dict(ma=32)), ("min_agree_negative", INV, dict(ma=-1)),
        ("max_conflict_32", INV, dict(mc=32)), ("max_conflict_negative", INV, dict(mc=-1)),
        ("out_sub_without_subpix", INV, dict(s=None)),
        ("out_is_disps", INV, dict(out="d")),
        ("out_in_disps", INV, dict(out=("d", 2 * np_ - 2))),
        ("out_before_disps", INV, dict(out=("d", -2))),
        ("out_in_subpix", INV, dict(out=("s", 4 * np_ - 2))),
        ("out_sub_is_subpix", INV, dict(osub="s")),
        ("out_sub_in_disps", INV, dict(osub=("d", 0))),
        ("too_many_pixels", UNS, dict(W=65536, H=32768)),
    ]
    ctx.set_timing(sva.SVA_TIMING_ALL)
    ctx.reset_timing()
    try:
        for host in (True, False):
            fn = sva.lib.sva_cross_check if host else sva.lib.sva_cross_check_d
            for name, status, ch in cases:
                b = host_buffers() if host else dev_buffers()
                p = ptrs_of(b, host)
                a = dict(p, n=n, W=W, H=H, steps=steps, md=1, ma=1, mc=0)
                for k, v in ch.items():
                    if k in ("out", "osub") and isinstance(v, str):
                        a[k] = p[v]
                    elif k in ("out", "osub") and isinstance(v, tuple):
                        a[k] = p[v[0]] + v[1]
                    else:
                        a[k] = v
                st = fn(ctx.h, a["d"], a["s"], a["n"], a["W"], a["H"],
                        sva._steps(a["steps"], max(a["n"], 1)), INVALID, a["md"], a["ma"], a["mc"],
                        a["out"], a["osub"], a["ag"], a["cf"])
                assert st == status, (name, host, st, sva.lib.sva_last_error(ctx.h))
                ctx.synchronize()
                torch.cuda.synchronize()
                if host:
                    assert np.array_equal(b["d"], d) and same32(b["s"], s), name
                    assert (b["out"] == 0x5A5A).all() and (b["osub"] == 7.0).all(), name
                    assert (b["ag"] == 0xEE).all() and (b["cf"] == 0xEE).all(), name
                else:
                    flat = b["flat"].cpu().numpy()
                    fsub = b["fsub"].cpu().numpy()
                    assert np.array_equal(flat[:np_].view(np.uint16), d.ravel()), name
                    assert (flat[np_:] == 0x5A5A).all(), name
                    assert same32(fsub[:np_], s.ravel()) and (fsub[np_:] == 7.0).all(), name
                    assert (b["cnt"].cpu().numpy() == 0xEE).all(), name
        assert ctx.kernel_time("cross_check")[1] == 0
    finally:
        ctx.set_timing(0)
