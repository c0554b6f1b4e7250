"""Expected values of the cross-view consistency check in
numpy: a vectorised loop over the view pairs (a, b).  No fixtures, no GPU calls."""
import numpy as np

NONE, AGREE, CONFLICT, OCCLUDED = 0, 1, 2, 3


def valid(d, invalid):
    d = np.asarray(d, dtype=np.int64)
    return (d != invalid) & (d != 0)


def target(px, py, s, ex, ey, W, H):
    """(qx, qy, inside) of q = p + s * e, elementwise on i64."""
    px, py, s = (np.asarray(v, dtype=np.int64) for v in (px, py, s))
    qx, qy = px + s * ex, py + s * ey
    return qx, qy, (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)


def classes(s, t, invalid, max_diff):
    """What a valid s meets in t, elementwise: NONE where t is not valid, AGREE
    where |t - s| <= max_diff, CONFLICT where t < s - max_diff, else OCCLUDED."""
    s, t = np.asarray(s, dtype=np.int64), np.asarray(t, dtype=np.int64)
    c = np.where(t - s < -max_diff, CONFLICT, np.where(t - s > max_diff, OCCLUDED, AGREE))
    return np.where(valid(t, invalid), c, NONE)


def counts(disps, view_step, invalid=0xFFFF, max_diff=1):
    """(agree, conflict), each [n][H][W] i64: how many other views agree with, and
    how many see through, every valid pixel (0 at the others)."""
    disps = np.asarray(disps, dtype=np.uint16)
    n, H, W = disps.shape
    steps = np.asarray(view_step, dtype=np.int64).reshape(-1, 2)[:n]
    yy, xx = np.mgrid[0:H, 0:W]
    agree = np.zeros((n, H, W), np.int64)
    conflict = np.zeros((n, H, W), np.int64)
    for a in range(n):
        s = disps[a].astype(np.int64)
        ok = valid(s, invalid)
        for b in range(n):
            if b == a:
                continue
            ex, ey = steps[b] - steps[a]
            qx, qy, ins = target(xx, yy, s, ex, ey, W, H)
            t = disps[b][np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
            c = np.where(ok & ins, classes(s, t, invalid, max_diff), NONE)
            agree[a] += c == AGREE
            conflict[a] += c == CONFLICT
    return agree, conflict


def decide(disps, agree, conflict, invalid=0xFFFF, min_agree=1, max_conflict=0, subpix=None):
    """(out u16, out_sub f32 or None, rejected bool) from the counts: a valid pixel
    stays where agree >= min_agree and conflict <= max_conflict, else it becomes
    `invalid` and NaN; the pixels that were not valid keep both values."""
    disps = np.asarray(disps, dtype=np.uint16)
    rejected = valid(disps, invalid) & ~((agree >= min_agree) & (conflict <= max_conflict))
    out = np.where(rejected, invalid, disps).astype(np.uint16)
    out_sub = None
    if subpix is not None:
        out_sub = np.array(subpix, dtype=np.float32, copy=True)
        out_sub[rejected] = np.nan
    return out, out_sub, rejected


def cross_check(disps, view_step, invalid=0xFFFF, max_diff=1, min_agree=1, max_conflict=0,
                subpix=None):
    """(out u16, out_sub f32 or None, agree u8, conflict u8), each [n][H][W]."""
    agree, conflict = counts(disps, view_step, invalid, max_diff)
    out, out_sub, _ = decide(disps, agree, conflict, invalid, min_agree, max_conflict, subpix)
    return out, out_sub, agree.astype(np.uint8), conflict.astype(np.uint8)
