"""Sub-pixel fusion without a GPU: the library exports the five
new entry points at the unchanged ABI version, and the numpy expectation the GPU
tests compare against (tests/sub_expect.py) gives hand-worked values, and, where
every sub-pixel disparity is its integer one, the depths of the u16 fusions."""
import re
import subprocess

import numpy as np

import conf_expect as ce
import sub_expect as se

NEW = ["sva_fuse_depth_sub", "sva_fuse_depth_sub_d", "sva_fuse_depth_conf_sub",
       "sva_fuse_depth_conf_sub_d", "sva_array_depth_sub"]
INVALID = 0xFFFF


def test_library_exports_the_new_entry_points(sva):
    out = subprocess.run(["nm", "-D", "--defined-only", sva.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (sva_[a-z0-9_]+)", out))
    assert not set(NEW) - exported
    assert set(NEW) <= set(sva.EXPORTED)
    assert sva.lib.sva_abi_version() == 6 == sva.ABI_VERSION
    assert (sva.SVA_ARRAY_PAIRS, sva.SVA_ARRAY_GROUPS, sva.SVA_ARRAY_GROUPS_MIXED) == (0, 1, 2)
    for name in ("fuse_depth_sub", "fuse_depth_sub_d", "fuse_depth_conf_sub",
                 "fuse_depth_conf_sub_d"):
        assert callable(getattr(sva.Context, name))
    assert callable(sva.Multi.array_depth_sub)


# 3 maps, 4 pixels.  b * f = (0.5, 1, 2) and pixel_size = 0.25, so z = num / (s / 4).
B, F, PS = [1.0, 2.0, 4.0], 0.5, 0.25
NAN = np.nan
#             odd: 3 valid   even: 2 valid    NaN on a valid d   no valid map
D = np.array([[[5, 5, 7, 0]],
              [[9, INVALID, 7, INVALID]],
              [[2, 3, 7, 9]]], np.uint16)
S = np.array([[[2.0, 0.5, NAN, 0.3]],
              [[1.0, NAN, 4.0, NAN]],
              [[16.0, 4.0, NAN, -1.0]]], np.float32)
CMIN = np.array([[[7, 4, 1, 1]], [[3, 1, 9, 1]], [[3, 4, 1, 1]]], np.uint16)
CSEC = np.array([[[9, 9, 99, 9]], [[4, 99, 10, 9]], [[8, 6, 99, 9]]], np.uint16)


def test_valid_rule():
    ok = se.valid(D, S, INVALID)
    assert ok[:, 0].tolist() == [[True, True, False, False], [True, False, True, False],
                                 [True, True, False, False]]
    # 0.0f, -0.0f and a negative value do not count; the smallest positive float does
    s = np.array([0.0, -0.0, -3.0, np.float32(1e-45), np.inf], np.float32).reshape(5, 1, 1)
    d = np.full((5, 1, 1), 4, np.uint16)
    assert se.valid(d, s, INVALID).ravel().tolist() == [False, False, False, True, True]


def test_median_by_hand():
    z, nv, win = se.fuse_expect(D, S, None, None, B, F, PS, INVALID, se.FUSE_MEDIAN)
    assert win is None
    # pixel 0: z = 0.5/0.5, 1/0.25, 2/4 = 1, 4, 0.5 -> the middle one, 1
    # pixel 1: z = 0.5/0.125, -, 2/1 = 4, 2 -> (2 + 4) / 2
    # pixel 2: only map 1 (the other s are NaN): 1/1
    # pixel 3: d = 0, invalid, and s = -1: nothing
    assert z[0].tolist() == [1.0, 3.0, 1.0, 0.0]
    assert nv[0].tolist() == [3, 2, 1, 0]
    assert not np.isnan(z).any()


def test_winner_by_hand():
    z, nv, win = se.fuse_expect(D, S, CMIN, CSEC, B, F, PS, INVALID, se.FUSE_MIN_COST)
    # pixel 0: costs 7, 3, 3 -> the tie goes to map 1; pixel 1: map 1 (cost 1) is
    # invalid, maps 0 and 2 tie at 4 -> map 0; pixel 2: maps 0 and 2 (cost 1) are NaN
    assert win[0].tolist() == [1, 0, 1, 0xFF]
    assert z[0].tolist() == [4.0, 4.0, 1.0, 0.0]
    assert nv[0].tolist() == [3, 2, 1, 0]
    z, nv, win = se.fuse_expect(D, S, CMIN, CSEC, B, F, PS, INVALID, se.FUSE_MAX_MARGIN)
    # margins: pixel 0: 2, 1, 5 -> map 2; pixel 1: 5, (98), 2 -> map 0; pixel 2: map 1
    assert win[0].tolist() == [2, 0, 1, 0xFF]
    assert z[0].tolist() == [0.5, 4.0, 1.0, 0.0]


def test_depth_expression_in_f64():
    """(b * f) / ((double)s * pixel_size): the float widened first, two roundings."""
    s = np.float32(6.3)
    b, f, ps = 0.15, 0.05, 0.036 / 640
    z, nv, _ = se.fuse_expect(np.full((1, 1, 1), 6, np.uint16), np.full((1, 1, 1), s, np.float32),
                              None, None, [b], f, ps, INVALID, se.FUSE_MEDIAN)
    assert z[0, 0] == (b * f) / (float(s) * ps) and nv[0, 0] == 1
    assert z[0, 0] != (b * f) / (6.3 * ps)


def test_integer_subpixel_maps_give_the_u16_fusions(oracle):
    """s == (float)d everywhere: sub_expect equals conf_expect.fuse_expect and the
    oracle's median bit for bit ((double)(float)d == (double)d for a u16)."""
    rng = np.random.RandomState(5)
    n, H, W = 6, 9, 31
    d = rng.randint(0, 65535, size=(n, H, W)).astype(np.uint16)
    d[rng.rand(n, H, W) < 0.2] = INVALID
    d[rng.rand(n, H, W) < 0.1] = 0
    d[:, 0, 0] = INVALID
    s = d.astype(np.float32)
    s[d == INVALID] = np.nan
    cmin = rng.randint(40, 48, size=(n, H, W)).astype(np.uint16)
    csec = (cmin + rng.randint(0, 8, size=(n, H, W))).astype(np.uint16)
    b = 0.05 * (1 + np.arange(n) % 5)
    f, ps = 0.05, 0.036 / 640
    for mode in (se.FUSE_MIN_COST, se.FUSE_MAX_MARGIN):
        ez, env, ew = ce.fuse_expect(d, cmin, csec, b, f, ps, INVALID, mode)
        z, nv, w = se.fuse_expect(d, s, cmin, csec, b, f, ps, INVALID, mode)
        assert np.array_equal(z.view(np.uint64), ez.view(np.uint64))
        assert np.array_equal(nv, env) and np.array_equal(w, ew)
    oz, onv = oracle.fuse_depth(d, list(b), f, ps)
    z, nv, _ = se.fuse_expect(d, s, None, None, b, f, ps, INVALID, se.FUSE_MEDIAN)
    assert np.array_equal(z.view(np.uint64), oz.view(np.uint64)) and np.array_equal(nv, onv)
    assert (nv == 0).any() and (nv % 2 == 0).any() and (nv % 2 == 1).any()
