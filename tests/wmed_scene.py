"""The banded scene of the weighted median's tests: the rig,
geometry, truth and per-view defects of tests/cross_scene.py with the foreground
drawn from intensities 160..255 and the background from 0..95, so that the image
knows where the surface ends.  No GPU calls; the expected maps come from the CPU
oracle exactly as cross_scene.matched makes them."""
import functools

import numpy as np

import cross_expect as ce
import cross_scene as cs
import mb_expect

W, H, D, DMIN = cs.W, cs.H, cs.D, cs.DMIN
PITCH_M, F, PS = cs.PITCH_M, cs.F, cs.PS
INVALID, GRID, VIEW_STEP, FG, BG = cs.INVALID, cs.GRID, cs.VIEW_STEP, cs.FG, cs.BG
INTERIOR, CHECK = cs.INTERIOR, cs.CHECK
groups, jobs = cs.groups, cs.jobs


@functools.lru_cache(maxsize=None)
def views_and_truth():
    """(the nine u8 views, truth [9][H][W] i64), read-only."""
    rng = np.random.RandomState(5)
    bg = rng.randint(0, 96, (H + 64, W + 64))
    fg = rng.randint(160, 256, (H + 64, W + 64))
    yy, xx = np.mgrid[0:H, 0:W]
    views, truth = [], []
    for a, (gx, gy) in enumerate(GRID):
        fx, fy = xx + FG * gx, yy + FG * gy
        on = (fy >= 32) & (fy < 64) & (fx >= 48) & (fx < 88)
        v = np.where(on, fg[fy + 32, fx + 32], bg[yy + BG * gy + 32, xx + BG * gx + 32])
        v = v.astype(np.uint8)
        r = np.random.RandomState(100 + a)
        for _ in range(5):
            y0 = r.randint(16, H - 28)
            x0 = r.randint(16, W - 28)
            v[y0:y0 + 12, x0:x0 + 12] = r.randint(0, 256, (12, 12))
        v = np.ascontiguousarray(v)
        v.setflags(write=False)
        views.append(v)
        truth.append(np.where(on, FG, BG))
    t = np.stack(truth).astype(np.int64)
    t.setflags(write=False)
    return views, t


def views():
    return views_and_truth()[0]


@functools.lru_cache(maxsize=None)
def matched():
    """(disp u16, sub f32), each [9][H][W]: every group's map from the CPU oracle --
    census, the pairs' cost volumes, their fusion, aggregate, wta.  Read-only."""
    import pyoracle as oracle
    cen = [oracle.census(v) for v in views()]
    pairs, gs = groups(False)
    disp, sub = [], []
    for g in range(9):
        ps = pairs[gs[g]:gs[g + 1]]
        steps = [(sx, sy) for _, _, sx, sy, _ in ps]
        Cs = [oracle.cost2(cen[a], cen[b], D, DMIN, sx, sy) for a, b, sx, sy, _ in ps]
        Cf = mb_expect.fuse(Cs, steps, DMIN)
        d, s = oracle.wta(oracle.aggregate(Cf, threads=8), DMIN, subpixel=True)
        disp.append(d)
        sub.append(s)
    out = np.stack(disp), np.stack(sub)
    for a in out:
        a.setflags(write=False)
    return out


def checked(max_diff=1, min_agree=2, max_conflict=8):
    """(out, out_sub, agree, conflict) expected of the frame: cross_expect on matched()."""
    d, s = matched()
    return ce.cross_check(d, VIEW_STEP, INVALID, max_diff, min_agree, max_conflict, s)


def quality(maps, truth=None):
    """(wrong, correct, holes) over the interior of all nine views: wrong = valid
    and |d - truth| > 1, correct = valid and not wrong."""
    t = (views_and_truth()[1] if truth is None else truth)[INTERIOR]
    m = np.asarray(maps)[INTERIOR].astype(np.int64)
    ok = ce.valid(m, INVALID)
    wrong = ok & (np.abs(m - t) > 1)
    return int(wrong.sum()), int((ok & ~wrong).sum()), int((~ok).sum())
