"""Rectification and masking (§2.5g) in numpy: the rule of
csrc/rectify_math.h operation by operation, sva_rectify_view_of in its documented
order, and the pieces of the rectified frame's stand-alone composition.  No GPU
calls.  Every f64 operation below is one numpy (or Python float) operation, so
each is rounded on its own, in the order the header fixes."""
import numpy as np

LIMIT = 1048576.0
OUTSIDE = np.iinfo(np.int32).min
FIELDS = ("cx", "cy", "fx", "fy", "k1", "k2", "p1", "p2", "k3")


def view(h=(1, 0, 0, 0, 1, 0, 0, 0, 1), cx=0.0, cy=0.0, fx=1.0, fy=1.0, dist=(0, 0, 0, 0, 0)):
    """A view as a dict: h (9 f64) and the nine scalars of sva_rectify_view."""
    v = dict(h=np.asarray(h, np.float64).ravel().copy(), cx=float(cx), cy=float(cy),
             fx=float(fx), fy=float(fy))
    v.update(zip(("k1", "k2", "p1", "p2", "k3"), (float(c) for c in dist)))
    return v


def flat(v):
    """The 18 doubles of sva_rectify_view, in the struct's order."""
    return np.concatenate([v["h"], [v[k] for k in FIELDS]]).astype(np.float64)


def source(v, W, H):
    """(sx, sy, inside) [H][W] of a view's output grid."""
    h = v["h"]
    y, x = np.mgrid[0:H, 0:W]
    x = x.astype(np.float64)
    y = y.astype(np.float64)
    with np.errstate(all="ignore"):
        w = (h[6] * x + h[7] * y) + h[8]
        u = ((h[0] * x + h[1] * y) + h[2]) / w
        vv = ((h[3] * x + h[4] * y) + h[5]) / w
        k1, k2, p1, p2, k3 = (np.float64(v[k]) for k in ("k1", "k2", "p1", "p2", "k3"))
        if k1 == 0 and k2 == 0 and p1 == 0 and p2 == 0 and k3 == 0:
            sx, sy = u, vv
        else:
            cx, cy, fx, fy = (np.float64(v[k]) for k in ("cx", "cy", "fx", "fy"))
            xn = (u - cx) / fx
            yn = (vv - cy) / fy
            xx = xn * xn
            yy = yn * yn
            xy = xn * yn
            r2 = xx + yy
            rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
            xd = (xn * rad + (2.0 * p1) * xy) + p2 * (r2 + 2.0 * xx)
            yd = (yn * rad + p1 * (r2 + 2.0 * yy)) + (2.0 * p2) * xy
            sx = xd * fx + cx
            sy = yd * fy + cy
        inside = (w > 0) & (sx > -LIMIT) & (sx < LIMIT) & (sy > -LIMIT) & (sy < LIMIT)
    return sx, sy, inside


def rectify_one(src, v, W, H, border=0):
    """(out u8, valid u8, map i32 [H][W][2]) of one view."""
    sh, sw = src.shape
    sx, sy, inside = source(v, W, H)
    with np.errstate(all="ignore"):
        qx = np.where(inside, np.rint(np.where(inside, sx, 0.0) * 32.0), 0).astype(np.int64)
        qy = np.where(inside, np.rint(np.where(inside, sy, 0.0) * 32.0), 0).astype(np.int64)
    X, a, Y, b = qx >> 5, qx & 31, qy >> 5, qy & 31
    total = np.full((H, W), 512, np.int64)
    valid = inside.copy()
    s = src.astype(np.int64)
    for dy, wy in ((0, 32 - b), (1, b)):
        for dx, wx in ((0, 32 - a), (1, a)):
            wt = wx * wy
            tx, ty = X + dx, Y + dy
            inn = (tx >= 0) & (tx < sw) & (ty >= 0) & (ty < sh)
            tap = np.where(inn, s[np.clip(ty, 0, sh - 1), np.clip(tx, 0, sw - 1)], border)
            total += wt * tap                      # a tap of weight 0 adds nothing
            valid &= inn | (wt == 0)
    out = np.where(inside, total >> 10, border).astype(np.uint8)
    qmap = np.stack([np.where(inside, qx, OUTSIDE), np.where(inside, qy, OUTSIDE)], -1)
    return out, valid.astype(np.uint8), qmap.astype(np.int32)


def rectify(srcs, views, size=None, border=0):
    """(out, valid, map) of n views [n][sh][sw]; size = (W, H), None: the source's."""
    srcs = np.asarray(srcs)
    W, H = (srcs.shape[2], srcs.shape[1]) if size is None else size
    r = [rectify_one(s, v, W, H, border) for s, v in zip(srcs, views)]
    return tuple(np.stack([q[i] for q in r]) for i in range(3))


def mask_maps(disps, valid, invalid, subpix=None):
    """(out, out_sub or None): sva_mask_maps."""
    out = np.where(valid != 0, disps, invalid).astype(np.uint16)
    if subpix is None:
        return out, None
    return out, np.where(valid != 0, subpix, np.float32(np.nan)).astype(np.float32)


# ---- sva_rectify_view_of, in rectify_math.h's order, on Python floats ----
def mul3(a, b):
    return [(a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j]
            for i in range(3) for j in range(3)]


def inv3(k):
    c = [k[4] * k[8] - k[5] * k[7], k[2] * k[7] - k[1] * k[8], k[1] * k[5] - k[2] * k[4],
         k[5] * k[6] - k[3] * k[8], k[0] * k[8] - k[2] * k[6], k[2] * k[3] - k[0] * k[5],
         k[3] * k[7] - k[4] * k[6], k[1] * k[6] - k[0] * k[7], k[0] * k[4] - k[1] * k[3]]
    det = (k[0] * c[0] + k[1] * c[3]) + k[2] * c[6]
    if not np.isfinite(det) or det == 0.0:
        return None
    return [ci / det for ci in c]


def view_of(K_raw, dist, R, K_ideal):
    """The view of a calibration, or None where sva_rectify_view_of refuses."""
    K_raw, dist, R, K_ideal = ([float(x) for x in np.asarray(a, np.float64).ravel()]
                               for a in (K_raw, dist, R, K_ideal))
    if not all(np.isfinite(x) for x in K_raw + dist + R + K_ideal):
        return None
    if K_raw[1] != 0 or K_raw[3] != 0 or K_raw[6] != 0 or K_raw[7] != 0 or K_raw[8] != 1:
        return None
    inv = inv3(K_ideal)
    if inv is None:
        return None
    return view(mul3(K_raw, mul3(R, inv)), K_raw[2], K_raw[5], K_raw[0], K_raw[4], dist)


# ---- test models ----
def rolled(W, H, roll_deg=0.7, shift=(2.0, -1.5), persp=(2e-5, -1e-5), k1=-0.12, k2=0.0,
           p1=0.0, p2=0.0, k3=0.0, f=None):
    """A view with a roll about the image centre, a shift, slight perspective terms
    and distortion about the centre: the "full model" of the tests."""
    f = float(f if f is not None else W)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    t = np.deg2rad(roll_deg)
    c, s = np.cos(t), np.sin(t)
    h = [c, -s, cx - c * cx + s * cy + shift[0], s, c, cy - s * cx - c * cy + shift[1],
         persp[0], persp[1], 1.0]
    return view(h, cx, cy, f, f, (k1, k2, p1, p2, k3))


def texture(W, H, seed):
    """A u8 image with structure at several scales."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    img = 96 + 60 * np.sin(x / 5.0 + seed) * np.cos(y / 7.0) + rng.integers(-40, 41, (H, W))
    return np.clip(img, 0, 255).astype(np.uint8)
