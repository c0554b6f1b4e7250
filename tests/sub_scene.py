"""The slanted-plane scene of the sub-pixel quality check (DESIGN.md §2.6c;
tests/test_array_sub_gpu.py): one reference view and its four neighbours one
grid unit away, the per-grid-unit disparity a plane from 6.0 to 14.0 across x.
No GPU calls."""
import functools

import numpy as np

W, H, D = 112, 80, 64
PITCH_M, F, PS = 0.05, 0.05, 0.036 / 160
GRID = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)]     # view 0 is the reference
INTERIOR = (slice(16, -16), slice(24, -24))
PAD = 16


def delta():
    """[W] f64: the disparity per grid unit at column x."""
    return 6.0 + 8.0 * np.arange(W) / (W - 1)


@functools.lru_cache(maxsize=None)
def views():
    """The five u8 views: bilinear samples of a smoothed random texture T at
    (x + gx * delta(x), y + gy * delta(x))."""
    rng = np.random.RandomState(11)
    T = rng.randint(0, 256, size=(H + 2 * PAD, W + 2 * PAD)).astype(np.float64)
    for _ in range(2):                      # [1 2 1] / 4 along both axes, edges clamped
        P = np.pad(T, 1, mode="edge")
        T = (P[:-2, 1:-1] + 2 * P[1:-1, 1:-1] + P[2:, 1:-1]) / 4
        P = np.pad(T, 1, mode="edge")
        T = (P[1:-1, :-2] + 2 * P[1:-1, 1:-1] + P[1:-1, 2:]) / 4
    T = (T - T.min()) * (255.0 / (T.max() - T.min()))      # the full u8 range again
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    dl = delta()[None, :]
    out = []
    for gx, gy in GRID:
        xs, ys = xx + gx * dl + PAD, yy + gy * dl + PAD
        x0, y0 = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
        fx, fy = xs - x0, ys - y0
        v = (T[y0, x0] * (1 - fx) * (1 - fy) + T[y0, x0 + 1] * fx * (1 - fy) +
             T[y0 + 1, x0] * (1 - fx) * fy + T[y0 + 1, x0 + 1] * fx * fy)
        a = np.ascontiguousarray(np.rint(v).astype(np.uint8))
        a.setflags(write=False)
        out.append(a)
    return out


def steps():
    """The match step of each neighbour: -(gx, gy)."""
    return [(-gx, -gy) for gx, gy in GRID[1:]]


def true_depth():
    """[H][W] f64: PITCH_M * F / (delta * PS)."""
    return np.repeat((PITCH_M * F / (delta() * PS))[None, :], H, 0)


def interior_error(depth):
    """Mean relative depth error over the interior."""
    t = true_depth()[INTERIOR]
    return float(np.mean(np.abs(depth[INTERIOR] - t) / t))
