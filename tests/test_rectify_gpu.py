"""sva_rectify(_d) and sva_mask_maps(_d) (§2.5g) on the
device: value, valid and map byte for byte tests/rectify_expect.py's, at every
base and pitch residue modulo 4, the padding between rows untouched; the host
twins; the refusals, in order, writing nothing."""
import numpy as np
import pytest
import torch

import rectify_expect as re_

pytestmark = pytest.mark.gpu

CANARY = 0xEE


def table(sva, views):
    return [sva.RectifyView.make(v["h"], v["cx"], v["cy"], v["fx"], v["fy"],
                                 [v[k] for k in ("k1", "k2", "p1", "p2", "k3")]) for v in views]


def models(sw, sh):
    """Three different models for one launch: full, affine, distortion-free
    perspective."""
    return [re_.rolled(sw, sh, roll_deg=0.7, k1=-0.12, k2=0.03, p1=1e-3, p2=-2e-3, k3=0.01, f=55.0),
            re_.rolled(sw, sh, roll_deg=-1.1, shift=(-3.25, 2.5), persp=(0, 0), k1=0.0),
            re_.rolled(sw, sh, roll_deg=0.2, shift=(6.0, 4.0), persp=(-3e-4, 2e-4), k1=0.0)]


def run_d(ctx, sva, dev, srcs, views, size=None, border=0, src_pad=0, out_pad=0, src_base=0,
          out_base=0, valid_base=None, want_valid=True, want_map=True):
    """sva_rectify_d on planes with the given pitch paddings and byte offsets from
    an aligned allocation; returns (out, valid, map) with the padding checked."""
    srcs = np.asarray(srcs)
    n, sh, sw = srcs.shape
    W, H = (sw, sh) if size is None else size
    sp, op = sw + src_pad, W + out_pad
    valid_base = out_base if valid_base is None else valid_base
    host = np.full((n, sh, sp), 0x11, np.uint8)
    host[:, :, :sw] = srcs
    tsrc = torch.zeros(n * sh * sp + src_base, dtype=torch.uint8, device=dev)
    tsrc[src_base:] = torch.from_numpy(host.ravel()).to(dev)
    tout = torch.full((n * H * op + out_base + 4,), CANARY, dtype=torch.uint8, device=dev)
    tval = torch.full((n * H * op + valid_base + 4,), CANARY, dtype=torch.uint8, device=dev)
    tmap = torch.full((n * H * W * 2 + 2,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    ctx.rectify_d(tsrc.data_ptr() + src_base, n, sw, sh, sp, table(sva, views), W, H, op, border,
                  tout.data_ptr() + out_base,
                  tval.data_ptr() + valid_base if want_valid else None,
                  tmap.data_ptr() if want_map else None)
    ctx.synchronize()
    torch.cuda.synchronize()
    res = []
    for t, base, used in ((tout, out_base, True), (tval, valid_base, want_valid)):
        a = t.cpu().numpy()
        assert (a[:base] == CANARY).all() and (a[base + n * H * op:] == CANARY).all()
        a = a[base:base + n * H * op].reshape(n, H, op)
        if used:
            # the last row's padding included: nothing past a row's W bytes is written
            assert (a[:, :, W:] == CANARY).all()
            res.append(np.ascontiguousarray(a[:, :, :W]))
        else:
            assert (a == CANARY).all()
            res.append(None)
    m = tmap.cpu().numpy()
    assert (m[n * H * W * 2:] == 0x5A5A5A5A).all()
    if want_map:
        res.append(m[:n * H * W * 2].reshape(n, H, W, 2))
    else:
        assert (m == 0x5A5A5A5A).all()
        res.append(None)
    return res


def same_as_expected(got, srcs, views, size, border):
    want = re_.rectify(srcs, views, size, border)
    for g, w, name in zip(got, want, ("out", "valid", "map")):
        if g is not None:
            assert np.array_equal(g, w), (name, int((g != w).sum()))
    return want


SRC3 = np.stack([re_.texture(61, 45, s) for s in (1, 2, 3)])


@pytest.mark.parametrize("pad,base", [(1, 0), (2, 1), (3, 2), (1, 3), (0, 0), (4, 2)])
def test_three_models_in_one_launch_at_every_alignment(ctx, sva, torch_dev, pad, base):
    """53 x 37 from 61 x 45, pitches W + 1 .. W + 3 and bases + 0 .. + 3 (valid at
    another residue than out): the dword groups, the byte edges, the padding."""
    got = run_d(ctx, sva, torch_dev, SRC3, models(61, 45), (53, 37), 200, src_pad=pad, out_pad=pad,
                src_base=(base + 1) % 4, out_base=base, valid_base=(base + pad) % 4)
    out, valid, _ = same_as_expected(got, SRC3, models(61, 45), (53, 37), 200)
    assert 0.5 < valid.mean() < 1.0 and len(np.unique(out)) > 100


def test_more_than_one_block_and_odd_width(ctx, sva, torch_dev):
    """A width past one workgroup's 256 pixels that is no multiple of 4, more rows
    than a workgroup's 4, output larger than the source."""
    src = re_.texture(150, 40, 7)[None]
    v = [re_.rolled(150, 40, roll_deg=2.0, shift=(-20.0, 3.0), persp=(1e-4, 0), k1=0.05, f=120.0)]
    # the scale: a 150 px source seen at 0.5 px steps
    v[0]["h"][[0, 1, 3, 4]] *= 0.5
    got = run_d(ctx, sva, torch_dev, src, v, (299, 21), 7, out_pad=3, out_base=1)
    same_as_expected(got, src, v, (299, 21), 7)


def test_one_pixel_output(ctx, sva, torch_dev):
    src = re_.texture(5, 4, 8)[None]
    v = [re_.view([1, 0, 2.25, 0, 1, 1.5, 0, 0, 1])]
    for base in range(4):
        got = run_d(ctx, sva, torch_dev, src, v, (1, 1), 0, out_base=base)
        same_as_expected(got, src, v, (1, 1), 0)
    assert got[1][0, 0, 0] == 1


def test_hand_checkable_cases(ctx, sva, torch_dev):
    src = re_.texture(23, 17, 9)[None]
    p = src[0].astype(int)
    out, valid, qmap = run_d(ctx, sva, torch_dev, src, [re_.view()])
    assert np.array_equal(out, src) and valid.all()
    assert np.array_equal(qmap[0, ..., 0], 32 * np.mgrid[0:17, 0:23][1])
    out, valid, _ = run_d(ctx, sva, torch_dev, src, [re_.view([1, 0, 5, 0, 1, -3, 0, 0, 1])],
                          border=77)
    want = np.full((17, 23), 77, np.uint8)
    want[3:, :18] = src[0, :14, 5:]
    assert np.array_equal(out[0], want)
    assert valid[0, 3:, :18].all() and valid.sum() == 14 * 18
    out, valid, _ = run_d(ctx, sva, torch_dev, src, [re_.view([1, 0, 0.5, 0, 1, 0, 0, 0, 1])])
    assert np.array_equal(out[0, :, :-1], (p[:, :-1] + p[:, 1:] + 1) >> 1)
    assert valid[0, :, :-1].all() and not valid[0, :, -1].any()


def test_outside_views_and_pixels(ctx, sva, torch_dev):
    """A view off the source, one behind the plane w = 0 on part of the frame, one
    that divides 0 by 0, one past the limits: border, valid 0, INT32_MIN."""
    src = np.stack([re_.texture(23, 17, 10)] * 4)
    views = [re_.view([1, 0, 500, 0, 1, 0, 0, 0, 1]), re_.view([1, 0, 0, 0, 1, 0, -0.125, 0, 1]),
             re_.view([1, 0, 0, 0, 1, 0, 1, 1, 0]), re_.view([1e300, 0, 0, 0, 1e300, 0, 0, 0, 1])]
    got = run_d(ctx, sva, torch_dev, src, views, border=41, out_pad=1)
    out, valid, qmap = same_as_expected(got, src, views, None, 41)
    assert not valid[0].any() and (out[0] == 41).all() and (qmap[0] != re_.OUTSIDE).all()
    assert (qmap[1][:, 8:] == re_.OUTSIDE).all() and (out[1][:, 8:] == 41).all()
    assert qmap[2][0, 0, 0] == re_.OUTSIDE and (qmap[3].reshape(-1, 2)[1:] == re_.OUTSIDE).all()


def test_widest_source_sampled_at_its_far_end(ctx, sva, torch_dev):
    """32767 x 4 into 64 x 4: the last tap column is the source's last."""
    src = np.random.default_rng(11).integers(0, 256, (1, 4, 32767)).astype(np.uint8)
    v = [re_.view([1, 0, 32703.25, 0, 1, 0.5, 0, 0, 1])]
    got = run_d(ctx, sva, torch_dev, src, v, (64, 4), 9)
    out, valid, qmap = same_as_expected(got, src, v, (64, 4), 9)
    assert valid[0, :3, :63].all() and not valid[0, :, 63].any() and not valid[0, 3].any()
    assert qmap[0, 0, 63, 0] == 32 * 32766 + 8


def test_more_views_than_one_launch_carries(ctx, sva, torch_dev):
    """27 views: the 26th and 27th go through a second launch with their own models."""
    src = np.stack([re_.texture(19, 11, 20 + i) for i in range(27)])
    views = [re_.rolled(19, 11, roll_deg=0.3 * i - 4, shift=(0.125 * i, -0.25 * i), persp=(0, 0),
                        k1=0.01 * (i % 3), f=30.0) for i in range(27)]
    got = run_d(ctx, sva, torch_dev, src, views, border=3, out_pad=1, out_base=3)
    same_as_expected(got, src, views, None, 3)


@pytest.mark.parametrize("want_valid,want_map", [(False, False), (True, False), (False, True)])
def test_null_planes(ctx, sva, torch_dev, want_valid, want_map):
    got = run_d(ctx, sva, torch_dev, SRC3, models(61, 45), (53, 37), 1, out_pad=2, out_base=1,
                want_valid=want_valid, want_map=want_map)
    same_as_expected(got, SRC3, models(61, 45), (53, 37), 1)


def test_host_entry_gives_the_device_entry_bytes(ctx, sva, torch_dev):
    rect = table(sva, models(61, 45))
    dev = run_d(ctx, sva, torch_dev, SRC3, models(61, 45), (53, 37), 200)
    out, valid, qmap = ctx.rectify(SRC3, rect, (53, 37), 200, want_valid=True, want_map=True)
    assert np.array_equal(out, dev[0]) and np.array_equal(valid, dev[1])
    assert np.array_equal(qmap, dev[2])
    bare = ctx.rectify(SRC3, rect, (53, 37), 200)
    assert np.array_equal(bare[0], out) and bare[1] is None and bare[2] is None
    # host pitches: rows apart at the caller's, the padding untouched
    n, sh, sw, W, H = 3, 45, 61, 53, 37
    src = np.full((n, sh, sw + 3), 0x11, np.uint8)
    src[:, :, :sw] = SRC3
    o = np.full((n, H, W + 2), CANARY, np.uint8)
    v = np.full((n, H, W + 2), CANARY, np.uint8)
    st = sva.lib.sva_rectify(ctx.h, src.ctypes.data, n, sw, sh, sw + 3, sva._view_table(rect), W, H,
                             W + 2, 200, o.ctypes.data, v.ctypes.data, None)
    assert st == 0
    assert np.array_equal(o[:, :, :W], out) and np.array_equal(v[:, :, :W], valid)
    assert (o[:, :, W:] == CANARY).all() and (v[:, :, W:] == CANARY).all()


def test_view_of_a_calibration_rectifies(ctx, sva):
    """sva.rectify_view mirrors the numpy form bit for bit and feeds ctx.rectify."""
    K_raw = [60.0, 0, 30.5, 0, 61.0, 21.5, 0, 0, 1]
    K_ideal = [58.0, 0, 30.0, 0, 58.0, 22.0, 0, 0, 1]
    c, s = np.cos(0.01), np.sin(0.01)
    R = [c, -s, 0, s, c, 0, 0, 0, 1]
    dist = [-0.1, 0.02, 1e-3, -1e-3, 0.0]
    got = sva.rectify_view(K_raw, dist, R, K_ideal)
    want = re_.view_of(K_raw, dist, R, K_ideal)
    flat = np.array(list(got.h) + [got.cx, got.cy, got.fx, got.fy, got.k1, got.k2, got.p1, got.p2,
                                   got.k3])
    assert np.array_equal(flat.view(np.uint64), re_.flat(want).view(np.uint64))
    out, valid, _ = ctx.rectify(SRC3[:1], [got], None, 5, want_valid=True)
    eo, ev, _ = re_.rectify(SRC3[:1], [want], None, 5)
    assert np.array_equal(out, eo) and np.array_equal(valid, ev) and valid.mean() > 0.8
    with pytest.raises(sva.SvaError):
        sva.rectify_view([60.0, 0.5, 30.5, 0, 61.0, 21.5, 0, 0, 1], dist, R, K_ideal)


def test_refusals_write_nothing(ctx, sva, torch_dev):
    """Every refusal of both entries, in the stated order: status, message,
    canary-filled outputs untouched, no kernel launched."""
    INV, UNS = sva.SVA_ERR_INVALID_ARG, sva.SVA_ERR_UNSUPPORTED
    n, sw, sh, W, H = 2, 20, 10, 16, 8
    nan = float("nan")
    good = dict(h=(1, 0, 0, 0, 1, 0, 0, 0, 1), cx=0.0, cy=0.0, fx=1.0, fy=1.0, dist=(0,) * 5)

    def views(**ch):
        a = [dict(good), dict(good)]
        for k, (i, v) in ch.items():
            a[i][k] = v
        return (sva.RectifyView * 2)(*[sva.RectifyView.make(**x) for x in a])

    # one allocation per plane: src leads it and a spare out follows, for the overlaps
    sizes = dict(src=n * sh * sw + n * H * W, out=n * H * W, valid=n * H * W, map=n * H * W * 8)
    cases = [
        ("null_src", INV, "null pointer", dict(src=None)),
        ("null_views", INV, "null pointer", dict(views=None)),
        ("null_out", INV, "null pointer", dict(out=None)),
        ("n_0", INV, "n must be", dict(n=0)),
        ("src_w_0", INV, "image size", dict(sw=0)), ("out_h_negative", INV, "image size", dict(H=-1)),
        ("src_h_32768", UNS, "32767", dict(sh=32768)), ("out_w_32768", UNS, "32767", dict(W=32768)),
        ("src_pitch", INV, "pitch < width", dict(sp=sw - 1)),
        ("out_pitch", INV, "pitch < width", dict(op=W - 1)),
        ("border_256", INV, "border", dict(border=256)),
        ("border_negative", INV, "border", dict(border=-1)),
        ("out_is_src", INV, "overlaps", dict(out=("src", 0))),
        ("out_on_src_end", INV, "overlaps", dict(out=("src", n * sh * sw - 1))),
        ("valid_in_out", INV, "overlaps", dict(valid=("out", 8))),
        ("map_in_src", INV, "overlaps", dict(map=("src", 16))),
        ("view_h", INV, "non-finite entry (view 1)", dict(views=views(h=(1, (1, 0, 0, 0, nan, 0, 0, 0, 1))))),
        ("view_c", INV, "cx, cy must be finite (view 0)", dict(views=views(cy=(0, float("inf"))))),
        ("view_f", INV, "fx, fy must be finite and > 0 (view 1)", dict(views=views(fx=(1, 0.0)))),
        ("view_k", INV, "coefficient is not finite (view 0)",
         dict(views=views(dist=(0, (0, 0, nan, 0, 0))))),
        # the order
        ("null_before_size", INV, "null pointer", dict(out=None, W=0)),
        ("size_before_unsupported", INV, "image size", dict(H=0, sw=40000)),
        ("unsupported_before_pitch", UNS, "32767", dict(sw=40000, sp=1)),
        ("pitch_before_border", INV, "pitch < width", dict(op=1, border=999)),
        ("border_before_overlap", INV, "border", dict(border=300, out=("src", 0))),
        ("overlap_before_views", INV, "overlaps", dict(out=("src", 0), views=views(fx=(0, -1.0)))),
        ("first_view_first", INV, "(view 0)", dict(views=views(fy=(0, nan), fx=(1, nan)))),
        ("h_before_f", INV, "non-finite entry (view 0)",
         dict(views=(sva.RectifyView * 2)(sva.RectifyView.make((nan,) * 9, fx=-1.0),
                                          sva.RectifyView.make()))),
    ]
    ok_views = views()
    ctx.set_timing(sva.SVA_TIMING_ALL)
    ctx.reset_timing()
    try:
        for host in (True, False):
            fn = sva.lib.sva_rectify if host else sva.lib.sva_rectify_d
            for name, status, text, ch in cases:
                b = {k: np.full(v, 0x5A, np.uint8) for k, v in sizes.items()}
                if not host:
                    b = {k: torch.from_numpy(v).to(torch_dev) for k, v in b.items()}
                base = {k: (v.ctypes.data if host else v.data_ptr()) for k, v in b.items()}
                at = lambda v: None if v is None else base[v[0]] + v[1]
                a = dict(src=("src", 0), n=n, sw=sw, sh=sh, sp=sw, views=ok_views, W=W, H=H, op=W,
                         border=0, out=("out", 0), valid=("valid", 0), map=("map", 0))
                a.update(ch)
                st = fn(ctx.h, at(a["src"]), a["n"], a["sw"], a["sh"], a["sp"], a["views"], a["W"],
                        a["H"], a["op"], a["border"], at(a["out"]), at(a["valid"]), at(a["map"]))
                msg = sva.lib.sva_last_error(ctx.h).decode()
                assert st == status and text in msg, (name, host, st, msg)
                ctx.synchronize()
                torch.cuda.synchronize()
                for k, v in b.items():
                    now = v if host else v.cpu().numpy()
                    assert (now == 0x5A).all(), (name, host, k)
        assert ctx.kernel_time("rectify")[1] == 0
        # the context still works, and one call of two views is one launch
        out, valid, _ = ctx.rectify(SRC3[:2], table(sva, models(61, 45)[:2]), want_valid=True)
        assert ctx.kernel_time("rectify")[1] == 1
    finally:
        ctx.set_timing(0)
    eo, ev, _ = re_.rectify(SRC3[:2], models(61, 45)[:2])
    assert np.array_equal(out, eo) and np.array_equal(valid, ev)


# ---- sva_mask_maps ----------------------------------------------------------------------
def mask_inputs(n=3, W=37, H=21, seed=5):
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 70, (n, H, W)).astype(np.uint16)
    d[rng.random((n, H, W)) < 0.1] = 0xFFFF
    s = (d.astype(np.float32) + rng.random((n, H, W), dtype=np.float32)).astype(np.float32)
    s[d == 0xFFFF] = np.nan
    valid = (rng.random((n, H, W)) < 0.7).astype(np.uint8) * rng.integers(1, 256, (n, H, W)).astype(np.uint8)
    return d, s, valid


def same32(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("with_sub", [False, True])
@pytest.mark.parametrize("invalid", [0xFFFF, 255])
def test_mask_maps_host(ctx, with_sub, invalid):
    d, s, valid = mask_inputs()
    eo, es = re_.mask_maps(d, valid, invalid, s if with_sub else None)
    out, osub = ctx.mask_maps(d, valid, invalid, s if with_sub else None)
    assert np.array_equal(out, eo) and (out[valid == 0] == invalid).all()
    assert 0.2 < (valid == 0).mean() < 0.4
    if with_sub:
        assert same32(osub, es) and np.isnan(osub[valid == 0]).all()
        assert same32(osub[valid != 0], s[valid != 0])
    else:
        assert osub is None


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("with_sub", [False, True])
def test_mask_maps_device(ctx, torch_dev, in_place, with_sub):
    d, s, valid = mask_inputs(n=2, W=41, H=13, seed=6)
    eo, es = re_.mask_maps(d, valid, 0xFFFF, s if with_sub else None)
    td = torch.from_numpy(d.view(np.int16).copy()).to(torch_dev)
    ts = torch.from_numpy(s.copy()).to(torch_dev) if with_sub else None
    tv = torch.from_numpy(valid.copy()).to(torch_dev)
    to = td if in_place else torch.full_like(td, 0x5A5A)
    tos = None if not with_sub else ts if in_place else torch.full_like(ts, 7.0)
    ptr = lambda t: None if t is None else t.data_ptr()
    ctx.mask_maps_d(ptr(td), ptr(ts), 2, 41, 13, ptr(tv), 0xFFFF, ptr(to), ptr(tos))
    ctx.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(to.cpu().numpy().view(np.uint16), eo)
    if with_sub:
        assert same32(tos.cpu().numpy(), es)
    if not in_place:
        assert np.array_equal(td.cpu().numpy().view(np.uint16), d)
    assert np.array_equal(tv.cpu().numpy(), valid)


def test_mask_maps_refusals(ctx, sva):
    INV, UNS = sva.SVA_ERR_INVALID_ARG, sva.SVA_ERR_UNSUPPORTED
    d, s, valid = mask_inputs(n=2, W=9, H=5)
    out, osub = np.full_like(d, 0x5A5A), np.full_like(s, 7.0)
    P = lambda a: None if a is None else a.ctypes.data
    cases = [("null_valid", INV, "null pointer", dict(valid=None, n=0)),
             ("null_out", INV, "null pointer", dict(out=None)),
             ("n_0", INV, "n_maps", dict(n=0, W=0)), ("size", INV, "image size", dict(H=0)),
             ("pixels", UNS, "2^31", dict(W=65536, H=32768, s=None)),
             ("out_sub_alone", INV, "out_sub needs subpix", dict(s=None)),
             ("out_shifted", INV, "overlaps", dict(out=d.ctypes.data + 2)),
             ("out_on_valid", INV, "overlaps", dict(out=valid.ctypes.data))]
    for name, status, text, ch in cases:
        a = dict(d=P(d), s=P(s), n=2, W=9, H=5, valid=P(valid), out=P(out), osub=P(osub))
        a.update(ch)
        for fn in (sva.lib.sva_mask_maps, sva.lib.sva_mask_maps_d):
            st = fn(ctx.h, a["d"], a["s"], a["n"], a["W"], a["H"], a["valid"], 0xFFFF, a["out"],
                    a["osub"])
            msg = sva.lib.sva_last_error(ctx.h).decode()
            assert st == status and text in msg, (name, st, msg)
    assert (out == 0x5A5A).all() and (osub == 7.0).all()
