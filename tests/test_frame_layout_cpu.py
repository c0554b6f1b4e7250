"""sva_frame_layout_of without a device: the plan a whole frame runs
(DESIGN.md §4.9a).  Expected sizes and offsets are the table's formulas,
restated here: vol = W*H*D, hck = 2*H*ceil(W/8)*D, vck = 2*ceil(H/8)*W*D,
hmn = 2*H*ceil(W/8)*8, vmn = 2*ceil(H/8)*W*8 at the native width D; the
checkpoint buffer holds hck, vck, on the pair route vck again, then hmn and
vmn where the D class has minima (128 in this build).  The pair route: native
D = 128, 2 * P2 <= 255 and W * H at or above the pixel threshold."""
import ctypes as ct

import pytest

PAIR, FOUR = 1, 0


def ceil_div(a, b):
    return -(-a // b)


def native(D):
    return 64 if D <= 64 else 128 if D <= 128 else 192 if D <= 192 else 256


def restated(W, H, D, pair):
    Dn = native(D)
    nsx, nsy = ceil_div(W, 8), ceil_div(H, 8)
    vol, hck, vck = W * H * Dn, 2 * H * nsx * Dn, 2 * nsy * W * Dn
    mn = Dn == 128
    hmn, vmn = (2 * H * nsx * 8, 2 * nsy * W * 8) if mn else (0, 0)
    pck = vck if pair else 0
    return dict(route=PAIR if pair else FOUR, minima=int(mn), D=Dn, seg=8, nsx=nsx, nsy=nsy,
                n_volumes=2 if pair else 4, cost_bytes=vol, volumes_bytes=(2 if pair else 4) * vol,
                ckpt_bytes=hck + vck + pck + hmn + vmn, hck_off=0, hck_bytes=hck, vck_off=hck,
                vck_bytes=vck, pair_off=hck + vck, pair_bytes=pck, hmn_off=hck + vck + pck,
                hmn_bytes=hmn, vmn_off=hck + vck + pck + hmn, vmn_bytes=vmn)


def fields(lay):
    return {name: getattr(lay, name) for name, _ in lay._fields_ if name != "reserved"}


# W, H, D, P2, pair_min_pixels, pair route expected
CASES = [
    (1920, 1080, 128, 127, -1, True),          # the flagship frame, built-in threshold
    (1920, 1080, 128, 128, -1, False),         # 2 * P2 does not fit a u8
    (1920, 1080, 128, 127, 1920 * 1080, True),
    (1920, 1080, 128, 127, 1920 * 1080 + 1, False),
    (65, 31, 128, 120, -1, False),             # below the built-in threshold
    (65, 31, 128, 120, 0, True),
    (65, 31, 128, 120, 65 * 31, True),
    (65, 31, 128, 120, 65 * 31 + 1, False),
    (65, 31, 100, 120, 0, True),               # padded D: planes of native width 128
    (65, 31, 65, 0, 0, True),
    (17, 9, 256, 120, 0, False),               # D classes without the pair route or minima
    (17, 9, 200, 120, 0, False),
    (17, 9, 64, 120, 0, False),
    (17, 9, 1, 120, 0, False),
    (17, 9, 129, 120, 0, False),
    (1, 1, 128, 127, 0, True),
]


@pytest.mark.parametrize("W,H,D,P2,thr,pair", CASES)
def test_layout_is_the_restated_table(sva, W, H, D, P2, thr, pair):
    p = sva.default_params(D=D, P2=P2)
    assert fields(sva.frame_layout(W, H, p, thr)) == restated(W, H, D, pair)


def test_flagship_numbers(sva):
    """1080p D = 128 on the pair route, written out."""
    lay = sva.frame_layout(1920, 1080, sva.default_params(D=128, P2=127))
    assert (lay.route, lay.minima, lay.n_volumes, lay.nsx, lay.nsy) == (PAIR, 1, 2, 240, 135)
    assert lay.volumes_bytes == 530841600
    assert (lay.hck_bytes, lay.vck_bytes, lay.pair_bytes) == (66355200,) * 3
    assert (lay.hmn_bytes, lay.vmn_bytes) == (4147200, 4147200)
    assert lay.ckpt_bytes == 3 * 66355200 + 2 * 4147200
    assert lay.hmn_off % 8 == 0 and lay.vmn_off % 8 == 0


def test_layout_ignores_what_the_plan_does_not_depend_on(sva):
    a = fields(sva.frame_layout(333, 77, sva.default_params(D=128), 0))
    b = fields(sva.frame_layout(333, 77, sva.default_params(D=128, P1=3, dmin=9, subpixel=1,
                                                            dir=1, lr_check=1), 0))
    assert a == b


def test_bad_arguments(sva):
    lib, out = sva.lib, sva.FrameLayout()
    p = sva.default_params(D=128)
    ok = lambda *a: lib.sva_frame_layout_of(*a)
    assert ok(65, 31, ct.byref(p), -1, ct.byref(out)) == sva.SVA_OK
    assert ok(65, 31, ct.byref(p), -1, None) == sva.SVA_ERR_INVALID_ARG
    assert ok(65, 31, None, -1, ct.byref(out)) == sva.SVA_ERR_INVALID_ARG
    assert ok(0, 31, ct.byref(p), -1, ct.byref(out)) == sva.SVA_ERR_INVALID_ARG
    assert ok(65, -1, ct.byref(p), -1, ct.byref(out)) == sva.SVA_ERR_INVALID_ARG
    for bad in (dict(D=0), dict(D=257), dict(P2=194), dict(P1=-1), dict(dmin=-1)):
        q = sva.default_params(**bad)
        assert ok(65, 31, ct.byref(q), -1, ct.byref(out)) == sva.SVA_ERR_INVALID_ARG, bad
    # W * H * D must stay below 2^32
    assert ok(65536, 512, ct.byref(p), -1, ct.byref(out)) == sva.SVA_ERR_INVALID_ARG
    # the two entries refuse a null context before anything else
    assert lib.sva_paths_frame_d(None, None, 0, 65, 31, ct.byref(p), None, 0, None, 0) == \
        sva.SVA_ERR_INVALID_ARG
    assert lib.sva_wta_frame_d(None, None, 0, None, 0, None, 0, 65, 31, ct.byref(p), 0, None, None,
                               None, None) == sva.SVA_ERR_INVALID_ARG
