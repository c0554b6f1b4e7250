"""Expected values of the sub-pixel fusion in numpy f64: the
counterpart of conf_expect.fuse_expect for sva_fuse_depth_sub* and
sva_fuse_depth_conf_sub*.  No fixtures, no GPU calls."""
import numpy as np

FUSE_MIN_COST, FUSE_MAX_MARGIN, FUSE_MEDIAN = 0, 1, 2


def valid(disps, sub, invalid):
    """Map i counts at a pixel iff d != invalid, d != 0 and s > 0.0f (false for NaN)."""
    d = np.asarray(disps, dtype=np.uint16)
    s = np.asarray(sub, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (d != invalid) & (d != 0) & (s > np.float32(0))


def depths(sub, baselines, f, pixel_size):
    """z_i = (b_i * f) / ((double)s_i * pixel_size), every map and pixel."""
    num = np.asarray(baselines, dtype=np.float64) * np.float64(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        return num[:, None, None] / (np.asarray(sub, np.float32).astype(np.float64) *
                                     np.float64(pixel_size))


def fuse_expect(disps, sub, cmin, csec, baselines, f, pixel_size, invalid, mode):
    """(depth f64, n_valid u8, winner u8 or None) of §2.6c.  mode FUSE_MEDIAN:
    the median of the valid depths (cmin, csec unused); FUSE_MIN_COST /
    FUSE_MAX_MARGIN: the depth of the winner of the §2.6b scan."""
    ok = valid(disps, sub, invalid)
    z = depths(sub, baselines, f, pixel_size)
    nv = ok.sum(axis=0).astype(np.uint8)
    if mode == FUSE_MEDIAN:
        zs = np.sort(np.where(ok, z, np.inf), axis=0)       # the valid depths first
        n = nv.astype(np.int64)
        lo = np.take_along_axis(zs, np.maximum((n - 1) >> 1, 0)[None], 0)[0]
        hi = np.take_along_axis(zs, np.minimum(n >> 1, zs.shape[0] - 1)[None], 0)[0]
        with np.errstate(invalid="ignore"):
            mid = (lo + hi) * 0.5
        depth = np.where(n == 0, 0.0, np.where(n & 1, lo, mid))
        return depth, nv, None
    if mode == FUSE_MIN_COST:
        score = np.asarray(cmin).astype(np.int64)
    else:   # the margin in unsigned 32-bit, negated: the largest wins
        score = -((np.asarray(csec).astype(np.uint32) -
                   np.asarray(cmin).astype(np.uint32)).astype(np.int64))
    score = np.where(ok, score, np.int64(1) << 40)
    win = score.argmin(axis=0)                  # the first of equal scores: lowest index
    zw = np.take_along_axis(z, win[None], 0)[0]
    depth = np.where(nv > 0, zw, 0.0)
    winner = np.where(nv > 0, win, 0xFF).astype(np.uint8)
    return depth, nv, winner
