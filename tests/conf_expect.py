"""Expected values of the WTA confidence planes, the uniqueness filter and the
cost-aware fusion, in numpy from the CPU oracle's S
volume, and the frames of tests/test_confidence_gpu.py.  No fixtures, no GPU
calls."""
import numpy as np

NONE = 0xFFFF          # cost_second when no disparity is further than 1 from d*
FUSE_MIN_COST, FUSE_MAX_MARGIN = 0, 1


def padded(D):
    return 64 if D <= 64 else 128 if D <= 128 else 192 if D <= 192 else 256


def conf_planes(S):
    """(d*, cost_min, cost_second) of S [H][W][D] u16 at the caller's D."""
    S = np.asarray(S, dtype=np.uint16)
    D = S.shape[2]
    ds = S.argmin(axis=2)                       # the first minimum
    cmin = S.min(axis=2).astype(np.uint16)
    near = np.abs(np.arange(D)[None, None, :] - ds[:, :, None]) <= 1
    csec = np.where(near, NONE, S).min(axis=2).astype(np.uint16)
    return ds, cmin, csec


def rejected(cmin, csec, u):
    """The uniqueness filter's predicate, in integers."""
    a = csec.astype(np.int64) * (100 - u)
    b = cmin.astype(np.int64) * 100
    return (csec != NONE) & (a < b)


def apply_filter(disp, sub, rej, invalid=0xFFFF):
    d = disp.copy()
    d[rej] = invalid
    s = None
    if sub is not None:
        s = sub.copy()
        s[rej] = np.nan
    return d, s


def frame(D, seed=7):
    """The confidence test frame: W = Dn + 51 (83 for D <= 8) x 41, uniform
    random L, R independent random and then R[:, x - d(x)] = L[:, x] with d
    constant on six column stripes {0, DPL-1, DPL, D/2, D-DPL, D-1} (clipped to
    [0, D-1], DPL = Dn / 16), and a constant 16 x 30 patch at rows 8-23 around
    column W/2, in R shifted left by D/2."""
    Dn = padded(D)
    dpl = Dn // 16
    W, H = (Dn + 51 if D > 8 else 83), 41
    rng = np.random.RandomState(1000 * seed + D)
    L = rng.randint(0, 256, size=(H, W)).astype(np.uint8)
    R = rng.randint(0, 256, size=(H, W)).astype(np.uint8)
    vals = np.clip(np.array([0, dpl - 1, dpl, D // 2, D - dpl, D - 1]), 0, D - 1)
    d = vals[(np.arange(W) * 6) // W]
    for x in range(W):
        if x - d[x] >= 0:
            R[:, x - d[x]] = L[:, x]
    x0 = W // 2 - 15
    L[8:24, x0:x0 + 30] = 128
    xr = max(0, x0 - D // 2)
    R[8:24, xr:xr + 30] = 128
    return np.ascontiguousarray(L), np.ascontiguousarray(R)


def check_coverage(D, ds, cmin, csec, shares=None):
    """The cases the frame must contain (asserted on the expected planes, so
    that an input change cannot empty one silently).  shares: {u: reject
    share} for D >= 64."""
    dpl = padded(D) // 16
    assert (ds == 0).sum() >= 200 and (ds == D - 1).sum() >= 200
    if D > 3:
        # d* on a lane's last / first disparity: d* + 1 / d* - 1 is another lane's
        assert ((ds % dpl == dpl - 1) & (ds + 1 < D)).any()
        assert ((ds % dpl == 0) & (ds > 0)).any()
    if D > 2:       # (at D <= 2 every d is within 1 of d*: no second cost to tie)
        assert (csec == cmin).sum() >= 12
    if D <= 3:
        assert (csec == NONE).any()
    else:
        assert (csec != NONE).all()
    assert (csec >= cmin).all()
    if D >= 64:
        for u, share in shares.items():
            assert 0.3 <= share <= 0.65, (u, share)


def fuse_expect(disps, cmin, csec, baselines, f, pixel_size, invalid, mode):
    """(depth f64, n_valid u8, winner u8) of §2.6b."""
    d = np.asarray(disps, dtype=np.uint16)
    N = d.shape[0]
    ok = (d != invalid) & (d != 0)
    if mode == FUSE_MIN_COST:
        score = cmin.astype(np.int64)
    else:   # the margin in unsigned 32-bit, negated: the largest wins
        score = -((csec.astype(np.uint32) - cmin.astype(np.uint32)).astype(np.int64))
    score = np.where(ok, score, np.int64(1) << 40)
    win = score.argmin(axis=0)                  # the first of equal scores: lowest index
    nv = ok.sum(axis=0).astype(np.uint8)
    dw = np.take_along_axis(d, win[None], 0)[0].astype(np.float64)
    num = (np.asarray(baselines, dtype=np.float64) * np.float64(f))[win]
    with np.errstate(divide="ignore", invalid="ignore"):
        z = num / (dw * np.float64(pixel_size))
    z = np.where(nv > 0, z, 0.0)
    winner = np.where(nv > 0, win, 0xFF).astype(np.uint8)
    return z, nv, winner
