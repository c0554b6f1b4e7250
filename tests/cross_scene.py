"""The scene of the cross-view check's array tests (DESIGN.md §2.5b;
tests/test_array_checked_gpu.py): a 3x3 rig looking at a fronto-parallel
foreground rectangle (disparity 10 per grid unit) before a background (4), and
in every view five 12x12 defects of its own -- dead blocks, glints -- that no
other view shares.  No GPU calls; the expected maps come from the CPU oracle."""
import functools
from math import gcd

import numpy as np

import cross_expect as ce
import mb_expect
import mixed_expect as mx

W, H, D, DMIN = 128, 96, 32, 0
PITCH_M, F, PS = 1.0, 0.05, 0.036 / 160        # pitch: metres per grid unit
INVALID = 0xFFFF
GRID = [(gx, gy) for gy in (-1, 0, 1) for gx in (-1, 0, 1)]
VIEW_STEP = [(-gx, -gy) for gx, gy in GRID]     # the match step a -> b is -(g_b - g_a)
FG, BG = 10, 4
INTERIOR = (slice(None), slice(12, -12), slice(12, -12))
CHECK = dict(max_diff=1, min_agree=2, max_conflict=8)       # the quality check's thresholds


@functools.lru_cache(maxsize=None)
def views_and_truth():
    """(the nine u8 views, truth [9][H][W] i64), read-only."""
    rng = np.random.RandomState(5)
    bg = rng.randint(0, 256, (H + 64, W + 64))
    fg = rng.randint(0, 256, (H + 64, W + 64))
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


def cheb(a, b):
    return max(abs(GRID[a][0] - GRID[b][0]), abs(GRID[a][1] - GRID[b][1]))


def step(a, b):
    """(sx, sy, k) of the pair (a, b): the reduced match step and its major baseline."""
    ex, ey = VIEW_STEP[b][0] - VIEW_STEP[a][0], VIEW_STEP[b][1] - VIEW_STEP[a][1]
    g = gcd(abs(ex), abs(ey))
    return ex // g, ey // g, cheb(a, b)


def groups(mixed=False):
    """(pairs [(ref, other, sx, sy, k)], group_start): group a = camera a against
    the cameras at Chebyshev distance 1 (mixed: against all eight), ascending."""
    pairs, gs = [], [0]
    for a in range(9):
        for b in range(9):
            if b != a and (mixed or cheb(a, b) == 1):
                pairs.append((a, b) + step(a, b))
        gs.append(len(pairs))
    return pairs, gs


def jobs(sva, mixed=False, **params):
    """(the (ref, other, SgmParams, baseline) jobs of Multi.array_depth*, group_start)."""
    pairs, gs = groups(mixed)
    return [(a, b, sva.default_params(D=D, dmin=DMIN, dir=sx, dir_y=sy, **params), k * PITCH_M)
            for a, b, sx, sy, k in pairs], gs


@functools.lru_cache(maxsize=None)
def matched(mixed=False):
    """(disp u16, sub f32), each [9][H][W]: every group's map from the CPU oracle --
    census, the pairs' cost volumes, their fusion, aggregate, wta.  Read-only."""
    import pyoracle as oracle
    cen = [oracle.census(v) for v in views()]
    pairs, gs = groups(mixed)
    disp, sub = [], []
    for g in range(9):
        ps = pairs[gs[g]:gs[g + 1]]
        steps = [(sx, sy) for _, _, sx, sy, _ in ps]
        if mixed:
            ratios = [mx.reduced(k, 1) for *_, k in ps]
            Cs = [mx.cost(cen[a], cen[b], D, DMIN, sx, sy, n, d)
                  for (a, b, sx, sy, _), (n, d) in zip(ps, ratios)]
            Cf = mx.fuse(Cs, steps, ratios, DMIN)
        else:
            Cs = [oracle.cost2(cen[a], cen[b], D, DMIN, sx, sy) for a, b, sx, sy, _ in ps]
            Cf = mb_expect.fuse(Cs, steps, DMIN)
        d, s = oracle.wta(oracle.aggregate(Cf, threads=8), DMIN, subpixel=True)
        disp.append(d)
        sub.append(s)
    out = np.stack(disp), np.stack(sub)
    for a in out:
        a.setflags(write=False)
    return out


def checked(mixed=False, max_diff=1, min_agree=2, max_conflict=8):
    """(out, out_sub, agree, conflict) expected of the frame: cross_expect on matched()."""
    d, s = matched(mixed)
    return ce.cross_check(d, VIEW_STEP, INVALID, max_diff, min_agree, max_conflict, s)


def quality(maps):
    """(wrong, correct) pixel counts over the interior of all nine views: wrong =
    valid and |d - truth| > 1, correct = valid and not wrong."""
    t = views_and_truth()[1][INTERIOR]
    m = np.asarray(maps)[INTERIOR].astype(np.int64)
    ok = ce.valid(m, INVALID)
    wrong = ok & (np.abs(m - t) > 1)
    return int(wrong.sum()), int((ok & ~wrong).sum())
