"""sva_weighted_median / sva_weighted_median_d on the
GPU: every output byte against tests/wmed_expect.py, at the frame sizes around
the kernel's tile and radii up to wider than the frame and the tile, guided and
unguided, on random maps of every hole share, an all-valid map and single
sources; the weight tables; fill, min_support and select (with tiles the kernel
skips); another `invalid`; pitched and 1-byte aligned guides, 2-byte aligned
maps; map independence, also past one launch's maps; the tie-breaks; absent
planes; the host twin and its staging across sizes; the refusals with nothing
written."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import fill_expect as fe
import wmed_expect as we

pytestmark = pytest.mark.gpu

INVALID = 0xFFFF
_TUNING = open(os.path.join(os.path.dirname(__file__), "..", "stereovisionarray_amd", "csrc",
                            "sva_tuning.h")).read()
TW, TH = (int(v) for v in re.search(r"kWmedTileW = (\d+), kWmedTileH = (\d+)", _TUNING).groups())
LAUNCH_MAPS = int(re.search(r"kWmedLaunchMaps = (\d+)", _TUNING).group(1))
# (W, H): one pixel, a row, a column, the tile -1, exactly and +1, several odd tiles
FRAMES = [(1, 1), (1, 9), (9, 1), (TW - 1, TH - 1), (TW, TH), (TW + 1, TH + 1), (193, 67)]
RADII = [1, 2, 7, 15]
frame_id = lambda f: "%dx%d" % f


def same32(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def tables():
    only_equal = np.zeros(256, np.uint16)
    only_equal[0] = 3
    return {"sigma8": we.weights(8), "only_equal": only_equal,
            "largest": np.full(256, 65535, np.uint16), "zero": np.zeros(256, np.uint16)}


@functools.lru_cache(maxsize=None)
def stack_of(W, H, seed=0, invalid=INVALID):
    """Six maps [6][H][W], their f32 planes and a guide each, read-only: random with
    10 %, 50 % and 100 % holes, all valid, one valid pixel in a corner, one in the
    centre.  Guides 0, 2, 4 have 256 levels, the others four (equal intensities)."""
    maps = [fe.random_map(W, H, 100 * W + H + seed, holes=h, invalid=invalid) for h in (0.1, 0.5)]
    maps.append(fe.random_map(W, H, 7, holes=1.1, invalid=invalid))
    maps.append(fe.random_map(W, H, 8, holes=0.0, invalid=invalid))
    for y, x in ((H - 1, 0), (H // 2, W // 2)):
        m = maps[2].copy()
        m[y, x] = 9
        maps.append(m)
    d = np.stack(maps)
    s = fe.subpix_of(d, seed)
    rng = np.random.default_rng(seed + 17)
    g = np.stack([rng.integers(0, (256, 4)[k % 2], (H, W)).astype(np.uint8) * (1, 60)[k % 2]
                  for k in range(6)])
    for a in (d, s, g):
        a.setflags(write=False)
    return d, s, g


@functools.lru_cache(maxsize=None)
def picks_of(W, H, r, table=None, seed=0, invalid=INVALID, n=6):
    d, _, g = stack_of(W, H, seed, invalid)
    if table is None:
        return we.picks(d[:n], invalid, r)
    return we.picks(d[:n], invalid, r, g[:n], tables()[table])


def dev16(a, dev, offset=0):
    flat = torch.zeros(a.size + offset, dtype=torch.int16, device=dev)
    flat[offset:] = torch.from_numpy(a.view(np.int16).ravel().copy()).to(dev)
    return flat[offset:]


def dev_guides(g, dev, pitch=None, offset=0):
    """(the tensor that owns them, the device address of every image, pitch): the
    images `pitch` bytes a row in one allocation that starts `offset` bytes early;
    the padding holds 0xEE."""
    n, H, W = g.shape
    pitch = W if pitch is None else pitch
    host = np.full((n, H, pitch), 0xEE, np.uint8)
    host[:, :, :W] = g
    flat = torch.full((host.size + offset,), 0xEE, dtype=torch.uint8, device=dev)
    flat[offset:] = torch.from_numpy(host.ravel()).to(dev)
    return flat, [flat.data_ptr() + offset + k * H * pitch for k in range(n)], pitch


def run_d(ctx, dev, d, r, g=None, w=None, s=None, sel=None, ms=1, fill=1, invalid=INVALID,
          want_sub=True, want_support=True, offset=0, pitch=None, g_offset=0):
    """(out, out_sub, support) of sva_weighted_median_d; absent outputs None."""
    n, H, W = d.shape
    td = dev16(d, dev, offset)
    ts = torch.from_numpy(s.copy()).to(dev) if s is not None else None
    tsel = torch.from_numpy(np.ascontiguousarray(sel, dtype=np.uint8)).to(dev) if sel is not None \
        else None
    own, gptr, gpitch = dev_guides(g, dev, pitch, g_offset) if g is not None else (None, None, 0)
    want_sub = want_sub and s is not None
    out = torch.full((d.size + offset,), 0x5A5A, dtype=torch.int16, device=dev)[offset:]
    osub = torch.full(d.shape, 7.0, device=dev) if want_sub else None
    sup = torch.full((d.size + offset,), 0x6B6B, dtype=torch.int16, device=dev)[offset:] \
        if want_support else None
    ptr = lambda t: None if t is None else t.data_ptr()
    ctx.weighted_median_d(ptr(td), ptr(ts), gptr, gpitch, w, ptr(tsel), n, W, H, invalid, r, ms,
                          fill, ptr(out), ptr(osub), ptr(sup))
    ctx.synchronize()
    torch.cuda.synchronize()
    del own
    return (out.cpu().numpy().view(np.uint16).reshape(d.shape),
            None if osub is None else osub.cpu().numpy().reshape(d.shape),
            None if sup is None else sup.cpu().numpy().view(np.uint16).reshape(d.shape))


def check(got, d, picked, r, s=None, sel=None, ms=1, fill=1, invalid=INVALID):
    out, osub, sup = got
    eo, es, en, written = we.apply(d, picked, invalid, r, s, sel, ms, fill)
    assert np.array_equal(out, eo), int((out != eo).sum())
    if osub is not None:
        assert same32(osub, es), int((osub.view(np.uint32) != es.view(np.uint32)).sum())
    if sup is not None:
        assert np.array_equal(sup, en), int((sup != en).sum())
    return written


@pytest.mark.parametrize("frame", FRAMES, ids=frame_id)
@pytest.mark.parametrize("r", RADII)
def test_frames_and_radii(ctx, torch_dev, r, frame):
    """Guided (sigma 8) and unguided, fill 0 and 1, min_support 1, 2, (2r + 1)^2
    and 961, on the six maps."""
    W, H = frame
    n = 3 if (r == 15 and W * H > 4096) else 6      # the expectation's sort, not the kernel
    d, s, g = (a[:n] for a in stack_of(W, H))
    full = (2 * r + 1) ** 2
    for table in ("sigma8", None):
        picked = picks_of(W, H, r, table, n=n)
        gw = dict(g=g, w=tables()[table]) if table else {}
        for ms, fill in ((1, 1), (2, 0), (full, 1), (961, 0), (full, 0)):
            written = check(run_d(ctx, torch_dev, d, r, s=s, ms=ms, fill=fill, **gw), d, picked, r,
                            s, None, ms, fill)
            assert not written[2].any()                     # all holes: no candidate anywhere
            if table is None and ms == 1 and fill == 1 and n == 6 and max(W, H) <= r + 1:
                assert written[4].all() and written[5].all()    # one source reaches every pixel
            if ms == 2 and n == 6:
                assert not written[4].any()


def test_the_cases_reach_every_outcome():
    """What the maps must contain for the comparisons to mean something."""
    W, H = FRAMES[-1]
    d, s, g = stack_of(W, H)
    hole = ~we.valid(d, INVALID)
    assert hole[2].all() and not hole[3].any() and hole[4].sum() == W * H - 1
    assert (d == 0).any() and (d == INVALID).any()
    guided, plain = picks_of(W, H, 2, "sigma8"), picks_of(W, H, 2)
    assert (guided[1] < plain[1]).any() and (guided[1] <= plain[1]).all()
    a = we.apply(d, guided, INVALID, 2, s, None, 1, 1)
    b = we.apply(d, plain, INVALID, 2, s, None, 1, 1)
    assert not np.array_equal(a[0], b[0])
    assert (a[3] & hole).any() and (a[3] & ~hole & (a[0] != d)).any()
    left = we.apply(d, guided, INVALID, 2, s, None, 25, 1)[3]
    assert left.any() and (~left & (guided[1] > 0)).any()
    # the interior of the all-valid map has full windows, unguided
    assert (plain[1][3] == 25).any() and (picks_of(W, H, 15)[1][3] == 961).any()


@pytest.mark.parametrize("table", ["only_equal", "largest", "zero"])
@pytest.mark.parametrize("r", [2, 15])
def test_weight_tables(ctx, torch_dev, r, table):
    """Zeros from delta 1 on (equal intensities only), all 65,535 (the largest
    sums: 961 * 65,535 at r = 15 on the all-valid map) and all zero (nothing is
    written and every count is 0)."""
    W, H = TW + 1, 4 * TH + 1
    assert W >= 31 and H >= 31
    d, s, g = stack_of(W, H)
    picked = picks_of(W, H, r, table)
    for fill in (0, 1):
        got = run_d(ctx, torch_dev, d, r, g, tables()[table], s, ms=1, fill=fill)
        written = check(got, d, picked, r, s, None, 1, fill)
        if table == "zero":
            assert not written.any() and not got[2].any() and np.array_equal(got[0], d)
            assert same32(got[1], s)
        else:
            assert written.any()
    if table == "only_equal":
        assert (picked[1][1] < picks_of(W, H, r)[1][1]).any()
    if table == "largest":
        assert np.array_equal(picked[1], picks_of(W, H, r)[1])
        assert r < 15 or picked[1][3].max() == 961


@pytest.mark.parametrize("guided", [False, True])
def test_select(ctx, torch_dev, guided):
    """No plane, all zero (every tile is skipped: a copy), random, and one lit
    tile among skipped ones whose pixels still read their neighbours' tiles."""
    W, H = 3 * TW + 1, 3 * TH + 1
    d, s, g = stack_of(W, H)
    r = 2
    picked = picks_of(W, H, r, "sigma8" if guided else None)
    gw = dict(g=g, w=tables()["sigma8"]) if guided else {}
    rng = np.random.default_rng(4)
    one_tile = np.zeros(d.shape, np.uint8)
    one_tile[:, TH:2 * TH, TW:2 * TW] = 200
    for sel in (None, np.zeros(d.shape, np.uint8), (rng.random(d.shape) < 0.3).astype(np.uint8),
                one_tile):
        for fill in (0, 1):
            got = run_d(ctx, torch_dev, d, r, s=s, sel=sel, ms=1, fill=fill, **gw)
            written = check(got, d, picked, r, s, sel, 1, fill)
            if sel is not None and not sel.any():
                assert not written.any() and np.array_equal(got[0], d) and same32(got[1], s)
                assert not got[2].any()
            if sel is one_tile:
                assert written[0].any() and not written[:, :TH].any()


def test_another_invalid(ctx, torch_dev):
    """invalid = 77: 0xFFFF is then a disparity like any other, and a large one."""
    W, H = TW + 1, TH + 1
    d, _, g = stack_of(W, H, 3, 77)
    d = d.copy()
    d[:, ::5, ::3] = 0xFFFF
    d[:, 1::5, ::3] = 0xFFFE
    s = fe.subpix_of(d, 2)
    for gw in (dict(), dict(g=g, w=tables()["sigma8"])):
        picked = we.picks(d, 77, 2, gw.get("g"), gw.get("w"))
        for fill in (0, 1):
            got = run_d(ctx, torch_dev, d, 2, s=s, fill=fill, invalid=77, **gw)
            check(got, d, picked, 2, s, None, 1, fill, invalid=77)
    assert (got[0] >= 0xFFFE).any() and (got[0][d == 77] != 77).any()


@pytest.mark.parametrize("frame", [(TW + 1, TH + 1), (3, 5), (1, 1)], ids=frame_id)
def test_views_pitch_and_alignment(ctx, torch_dev, frame):
    """A guide pitch larger than the width, guides that start at an odd byte, and
    u16 planes one element into a larger tensor (2-byte aligned only)."""
    W, H = frame
    d, s, g = stack_of(W, H)
    picked = picks_of(W, H, 2, "sigma8")
    w = tables()["sigma8"]
    for kw in (dict(pitch=W + 5), dict(g_offset=1), dict(pitch=W + 3, g_offset=3), dict(offset=1),
               dict(offset=1, pitch=W + 1, g_offset=1)):
        check(run_d(ctx, torch_dev, d, 2, g, w, s, ms=2, **kw), d, picked, 2, s, None, 2, 1)


def test_maps_do_not_interact(ctx, torch_dev):
    """Six maps, a guide each; map k is map 0 rolled and raised: a value, or a
    guide, leaking between maps shows.  Each map alone gives its plane of the six."""
    W, H = TW + 1, TH + 1
    d0 = fe.random_map(W, H, 5, holes=0.4)
    maps = []
    for k in range(6):
        m = np.roll(d0, (k, 2 * k), axis=(0, 1)).copy()
        m[we.valid(m, INVALID)] += 50 * k
        maps.append(m)
    d = np.stack(maps)
    s = fe.subpix_of(d, 1)
    g = stack_of(W, H)[2]
    w = tables()["sigma8"]
    got = run_d(ctx, torch_dev, d, 3, g, w, s, ms=2)
    check(got, d, we.picks(d, INVALID, 3, g, w), 3, s, None, 2, 1)
    for k in range(6):
        alone = run_d(ctx, torch_dev, d[k:k + 1], 3, g[k:k + 1], w, s[k:k + 1], ms=2)
        assert np.array_equal(alone[0][0], got[0][k]) and same32(alone[1][0], got[1][k])
        assert np.array_equal(alone[2][0], got[2][k])
        ok = we.valid(got[0][k], INVALID)
        assert (got[0][k][ok] > 50 * k).all() and (got[0][k][ok] <= 50 * k + 40).all()


def test_more_maps_than_one_launch_carries(ctx, torch_dev):
    """kWmedLaunchMaps + 3 small maps with a guide each: the later launches take
    their own maps, guides, select and outputs."""
    n, W, H = LAUNCH_MAPS + 3, 9, 5
    rng = np.random.default_rng(9)
    d = np.stack([fe.random_map(W, H, 300 + k, holes=0.3) for k in range(n)])
    g = rng.integers(0, 4, d.shape).astype(np.uint8) * 50
    s = fe.subpix_of(d, 4)
    sel = (rng.random(d.shape) < 0.7).astype(np.uint8)
    w = tables()["sigma8"]
    check(run_d(ctx, torch_dev, d, 2, g, w, s, sel), d, we.picks(d, INVALID, 2, g, w), 2, s, sel)
    check(run_d(ctx, torch_dev, d, 2, s=s), d, we.picks(d, INVALID, 2), 2, s)


def test_tie_breaks(ctx, torch_dev):
    """Equal d at several window positions with distinct subpix: out_sub names the
    source, the first in raster order at which the running weight reaches half."""
    d = np.zeros((3, 7, 7), np.uint16)
    s = np.arange(3 * 49, dtype=np.float32).reshape(3, 7, 7) + 0.25
    g = np.zeros((3, 7, 7), np.uint8)
    # map 0: four 5s around the hole (3, 3), flat weights: T = 4, the second in raster order
    for y, x in ((1, 3), (3, 1), (3, 5), (5, 3)):
        d[0, y, x] = 5
    # map 1: the same, but the first in raster order carries weight 3 of T = 6 itself
    d[1] = d[0]
    g[1, 1, 3] = 10                     # the centre (3, 3) has g = 10 too, the others 0
    g[1, 3, 3] = 10
    # map 2: values 4, 4, 9: T = 3, the second 4 crosses; 9 lies before them in raster order
    d[2, 0, 0], d[2, 2, 2], d[2, 2, 6] = 9, 4, 4
    w = np.ones(256, np.uint16)
    w[0] = 3
    got = run_d(ctx, torch_dev, d, 3, g, w, s)
    check(got, d, we.picks(d, INVALID, 3, g, w), 3, s)
    out, osub, sup = got
    assert out[0, 3, 3] == 5 and osub[0, 3, 3] == s[0, 3, 1] and sup[0, 3, 3] == 4
    assert out[1, 3, 3] == 5 and osub[1, 3, 3] == s[1, 1, 3]
    assert out[2, 3, 3] == 4 and osub[2, 3, 3] == s[2, 2, 6] and sup[2, 3, 3] == 3
    plain = run_d(ctx, torch_dev, d, 3, s=s)
    check(plain, d, we.picks(d, INVALID, 3), 3, s)
    assert plain[1][1, 3, 3] == s[1, 3, 1]


@pytest.mark.parametrize("want_sub,want_support,with_sub", [
    (True, True, True), (True, False, True), (False, True, True), (False, False, True),
    (False, True, False), (False, False, False)])
def test_absent_outputs(ctx, torch_dev, want_sub, want_support, with_sub):
    W, H = TW + 1, TH + 1
    d, s, g = stack_of(W, H)
    for table in ("sigma8", None):
        gw = dict(g=g, w=tables()[table]) if table else {}
        got = run_d(ctx, torch_dev, d, 2, s=s if with_sub else None, ms=2, want_sub=want_sub,
                    want_support=want_support, **gw)
        assert (got[1] is not None) == (want_sub and with_sub)
        assert (got[2] is not None) == want_support
        check(got, d, picks_of(W, H, 2, table), 2, s if with_sub else None, None, 2, 1)


def test_host_twin_and_staging_across_sizes(ctx, sva, torch_dev):
    """sva_weighted_median equals the device entry: a large frame, smaller ones in
    the kept staging buffers, the large one again; views as guides; one launch."""
    w = tables()["sigma8"]
    assert np.array_equal(sva.wmed_weights(8), w) and sva.SVA_WMED_MAX_RADIUS == 15
    for W, H in (FRAMES[-1], FRAMES[4], (7, 3), (1, 1), FRAMES[-1]):
        d, s, g = stack_of(W, H)
        sel = (np.random.default_rng(W).random(d.shape) < 0.5).astype(np.uint8)
        dev = run_d(ctx, torch_dev, d, 2, g, w, s, sel, ms=2)
        check(dev, d, picks_of(W, H, 2, "sigma8"), 2, s, sel, 2, 1)
        wide = np.full((6, H, W + 3), 0xEE, np.uint8)
        wide[:, :, :W] = g
        ctx.set_timing(sva.SVA_TIMING_ALL)
        ctx.reset_timing()
        try:
            host = ctx.weighted_median(d, 2, [wide[k, :, :W] for k in range(6)], w, s, sel, 2, 1)
            assert ctx.kernel_time("wmed")[1] == 1
        finally:
            ctx.set_timing(0)
        for a, b in zip(host, dev):
            assert same32(a, b) if a.dtype == np.float32 else np.array_equal(a, b)
        bare = ctx.weighted_median(d, 2, min_support=2, fill=0, want_support=False)
        assert bare[1] is None and bare[2] is None
        assert np.array_equal(bare[0], we.apply(d, picks_of(W, H, 2), INVALID, 2, None, None, 2, 0)[0])


def test_argument_errors_write_nothing(ctx, sva, torch_dev):
    """Every refusal of both entries, in the stated order: the status,
    canary-filled outputs untouched and no kernel launched."""
    W, H = TW + 1, TH + 1
    d, s, g = (a[:2] for a in stack_of(W, H))
    n = 2
    INV, UNS = sva.SVA_ERR_INVALID_ARG, sva.SVA_ERR_UNSUPPORTED
    np_ = n * W * H
    weights = tables()["sigma8"]

    def host_buffers():
        b = dict(d=np.zeros(2 * np_, np.uint16), s=np.zeros(2 * np_, np.float32),
                 sup=np.full(np_, 0x6B6B, np.uint16), sel=np.ones(np_, np.uint8),
                 g=np.zeros(np_ + 8, np.uint8))
        b["d"][:np_], b["d"][np_:] = d.ravel(), 0x5A5A
        b["s"][:np_], b["s"][np_:] = s.ravel(), 7.0
        b["g"][:np_] = g.ravel()
        return b

    def dev_buffers():
        return {k: torch.from_numpy(v.view({1: np.uint8, 2: np.int16, 4: np.int32}[v.itemsize]).copy())
                .to(torch_dev) for k, v in host_buffers().items()}

    def base_of(b, host):
        return {k: (v.ctypes.data if host else v.data_ptr()) for k, v in b.items()}

    # (plane, byte offset) names a pointer; the inputs lead their allocations,
    # the outputs follow them
    OUT, OSUB, SUP = ("d", 2 * np_), ("s", 4 * np_), ("sup", 0)
    G = [("g", 0), ("g", W * H)]
    cases = [
        ("null_disps", INV, "null pointer", dict(d=None)),
        ("null_out", INV, "null pointer", dict(out=None)),
        ("n_0", INV, "n_maps", dict(n=0)), ("n_negative", INV, "n_maps", dict(n=-1)),
        ("zero_width", INV, "image size", dict(W=0)),
        ("negative_height", INV, "image size", dict(H=-1)),
        ("too_many_pixels", UNS, "2^31", dict(W=65536, H=32768)),
        ("radius_0", INV, "radius", dict(r=0)), ("radius_16", INV, "radius", dict(r=16)),
        ("min_support_0", INV, "min_support", dict(ms=0)),
        ("min_support_962", INV, "min_support", dict(ms=962)),
        ("fill_negative", INV, "fill", dict(fill=-1)), ("fill_2", INV, "fill", dict(fill=2)),
        ("guides_without_weights", INV, "go together", dict(w=False)),
        ("weights_without_guides", INV, "go together", dict(g=None)),
        ("null_guide", INV, "null guide", dict(g=[G[0], None])),
        ("pitch_below_width", INV, "guide pitch", dict(pitch=W - 1)),
        ("out_sub_without_subpix", INV, "out_sub needs subpix", dict(s=None)),
        ("out_is_disps", INV, "overlaps", dict(out=("d", 0))),
        ("out_in_disps", INV, "overlaps", dict(out=("d", 2))),
        ("out_before_disps_end", INV, "overlaps", dict(out=("d", 2 * np_ - 2))),
        ("out_in_subpix", INV, "overlaps", dict(out=("s", 0))),
        ("out_in_select", INV, "overlaps", dict(out=("sel", 0))),
        ("out_in_a_guide", INV, "overlaps", dict(out=("g", 2 * W * H - 2))),
        ("out_in_out_sub", INV, "overlaps", dict(out=("s", 4 * np_ + 4))),
        ("out_in_support", INV, "overlaps", dict(out=("sup", 8))),
        ("out_sub_in_disps", INV, "overlaps", dict(osub=("d", 0))),
        ("out_sub_is_subpix", INV, "overlaps", dict(osub=("s", 0))),
        ("out_sub_in_support", INV, "overlaps", dict(osub=("sup", 0))),
        ("support_in_disps", INV, "overlaps", dict(sup=("d", 0))),
        ("support_in_select", INV, "overlaps", dict(sup=("sel", 0))),
        ("support_in_a_guide", INV, "overlaps", dict(sup=("g", 0))),
        # the order: each of these breaks the rule named first and later ones too
        ("null_before_size", INV, "null pointer", dict(d=None, W=0, r=0)),
        ("n_before_size", INV, "n_maps", dict(n=0, H=0)),
        ("size_before_unsupported", INV, "image size", dict(W=-1, H=2 ** 31 - 1, r=99)),
        ("unsupported_before_radius", UNS, "2^31", dict(W=65536, H=32768, r=16)),
        ("radius_before_min_support", INV, "radius", dict(r=16, ms=0, fill=2)),
        ("min_support_before_fill", INV, "min_support", dict(ms=962, fill=2, w=False)),
        ("fill_before_guides", INV, "fill", dict(fill=2, w=False)),
        ("pairing_before_null_guide", INV, "go together", dict(w=False, g=[None, None])),
        ("null_guide_before_pitch", INV, "null guide", dict(g=[None, G[1]], pitch=1)),
        ("pitch_before_out_sub", INV, "guide pitch", dict(pitch=0, s=None)),
        ("out_sub_before_overlap", INV, "out_sub needs subpix", dict(s=None, out=("d", 2))),
    ]
    ctx.set_timing(sva.SVA_TIMING_ALL)
    ctx.reset_timing()
    try:
        for host in (True, False):
            fn = sva.lib.sva_weighted_median if host else sva.lib.sva_weighted_median_d
            for name, status, text, ch in cases:
                b = host_buffers() if host else dev_buffers()
                base = base_of(b, host)
                at = lambda v: None if v is None else base[v[0]] + v[1]
                a = dict(d=("d", 0), s=("s", 0), sel=("sel", 0), g=G, w=True, pitch=W, out=OUT,
                         osub=OSUB, sup=SUP, n=n, W=W, H=H, r=2, ms=1, fill=1)
                a.update(ch)
                garr = None if a["g"] is None else (sva.ct.c_void_p * 2)(*[at(v) for v in a["g"]])
                st = fn(ctx.h, at(a["d"]), at(a["s"]), garr, a["pitch"],
                        weights.ctypes.data if a["w"] else None, at(a["sel"]), a["n"], a["W"],
                        a["H"], INVALID, a["r"], a["ms"], a["fill"], at(a["out"]), at(a["osub"]),
                        at(a["sup"]))
                msg = sva.lib.sva_last_error(ctx.h).decode()
                assert st == status and text in msg, (name, host, st, msg)
                ctx.synchronize()
                torch.cuda.synchronize()
                now = b if host else {k: v.cpu().numpy() for k, v in b.items()}
                ref = host_buffers()
                for k in ref:
                    assert np.array_equal(now[k].view(np.uint8), ref[k].view(np.uint8)), (name, k)
        assert ctx.kernel_time("wmed")[1] == 0
    finally:
        ctx.set_timing(0)
    # the context still works
    check(run_d(ctx, torch_dev, d, 2, g, weights, s), d, we.picks(d, INVALID, 2, g, weights), 2, s)
