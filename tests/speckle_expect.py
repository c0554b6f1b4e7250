"""The speckle filter's rule in numpy and plain Python: what
sva_filter_speckles* must produce, byte for byte.  A flood fill over the link
graph -- not the kernel's passes (tiles, label equivalence) -- and, for frames
of at most 4x4, a transitive closure of the link matrix to check the flood fill
itself (tests/test_speckle_cpu.py)."""
import numpy as np

MAX_DIFF = 65535


def valid(d, invalid):
    d = np.asarray(d)
    return (d != invalid) & (d != 0)


def links(d, invalid, max_diff):
    """(right [H][W-1], down [H-1][W]) bool: pixel (y, x) is linked to (y, x + 1)
    / (y + 1, x)."""
    md = min(int(max_diff), MAX_DIFF)
    v = np.asarray(d).astype(np.int64)
    ok = valid(v, invalid)
    right = ok[:, :-1] & ok[:, 1:] & (np.abs(v[:, :-1] - v[:, 1:]) <= md)
    down = ok[:-1, :] & ok[1:, :] & (np.abs(v[:-1, :] - v[1:, :]) <= md)
    return right, down


def comp_size_map(d, invalid, max_diff):
    """comp_size [H][W] u32 of one map: a flood fill from every unvisited valid pixel."""
    d = np.asarray(d)
    H, W = d.shape
    right, down = links(d, invalid, max_diff)
    # per pixel, as plain lists: linked to the right / to the pixel below
    r = np.zeros((H, W), bool)
    r[:, :-1] = right
    b = np.zeros((H, W), bool)
    b[:-1, :] = down
    r, b = r.ravel().tolist(), b.ravel().tolist()
    ok = valid(d, invalid).ravel().tolist()
    seen = [False] * (H * W)
    size = [0] * (H * W)
    for seed in range(H * W):
        if seen[seed] or not ok[seed]:
            continue
        seen[seed] = True
        stack, members = [seed], []
        while stack:
            p = stack.pop()
            members.append(p)
            if r[p] and not seen[p + 1]:
                seen[p + 1] = True
                stack.append(p + 1)
            if p % W and r[p - 1] and not seen[p - 1]:
                seen[p - 1] = True
                stack.append(p - 1)
            if b[p] and not seen[p + W]:
                seen[p + W] = True
                stack.append(p + W)
            if p >= W and b[p - W] and not seen[p - W]:
                seen[p - W] = True
                stack.append(p - W)
        for p in members:
            size[p] = len(members)
    return np.array(size, np.uint32).reshape(H, W)


def comp_size(disps, invalid, max_diff):
    """comp_size of maps [n][H][W] (or one [H][W]); maps never connect."""
    d = np.asarray(disps)
    if d.ndim == 2:
        return comp_size_map(d, invalid, max_diff)
    return np.stack([comp_size_map(m, invalid, max_diff) for m in d])


def apply(disps, size, invalid, max_size, subpix=None):
    """(out, out_sub or None, removed) from comp_size."""
    d = np.asarray(disps)
    gone = (size != 0) & (size.astype(np.int64) <= int(max_size))
    out = np.where(gone, np.uint16(invalid), d).astype(np.uint16)
    osub = None
    if subpix is not None:
        osub = np.where(gone, np.float32(np.nan), np.asarray(subpix)).astype(np.float32)
    return out, osub, gone


def filter_speckles(disps, invalid, max_size, max_diff, subpix=None):
    """(out, out_sub or None, comp_size) expected of sva_filter_speckles."""
    size = comp_size(disps, invalid, max_diff)
    out, osub, _ = apply(disps, size, invalid, max_size, subpix)
    return out, osub, size


def closure_size(d, invalid, max_diff):
    """comp_size of one small map from the transitive closure of its link matrix."""
    d = np.asarray(d)
    H, W = d.shape
    right, down = links(d, invalid, max_diff)
    ok = valid(d, invalid).ravel()
    A = np.diag(ok)
    for y in range(H):
        for x in range(W):
            p = y * W + x
            if x + 1 < W and right[y, x]:
                A[p, p + 1] = A[p + 1, p] = True
            if y + 1 < H and down[y, x]:
                A[p, p + W] = A[p + W, p] = True
    while True:
        B = A | ((A.astype(np.int64) @ A.astype(np.int64)) > 0)
        if np.array_equal(A, B):
            break
        A = B
    return A.sum(axis=1).astype(np.uint32).reshape(H, W)


# ---- the frames both test files use -------------------------------------------
def snake(W, H, value=9):
    """A one-pixel-wide path: every other row is full, joined to the next full
    row alternately at the right and the left end.  One component that crosses
    every vertical tile border in every full row."""
    d = np.zeros((H, W), np.uint16)
    for k, y in enumerate(range(0, H, 2)):
        d[y, :] = value
        if y + 1 < H and y + 2 < H:
            d[y + 1, W - 1 if k % 2 == 0 else 0] = value
    return d


def spiral(W, H, value=9):
    """A one-pixel-wide rectangular spiral with a one-pixel gap between its arms:
    walk ahead while the cell after the next one is free, else turn right."""
    d = np.zeros((H, W), np.uint16)
    x, y, dx, dy = 0, 0, 1, 0
    d[0, 0] = value

    def free(px, py):
        return not (0 <= px < W and 0 <= py < H) or d[py, px] == 0

    turns = 0
    while turns < 2:
        nx, ny = x + dx, y + dy
        if 0 <= nx < W and 0 <= ny < H and d[ny, nx] == 0 and free(nx + dx, ny + dy):
            x, y = nx, ny
            d[y, x] = value
            turns = 0
        else:
            dx, dy = -dy, dx
            turns += 1
    return d


def checkerboard(W, H, a=5, b=7):
    """Two values alternating: at max_diff 0 every pixel is its own component."""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where((yy + xx) % 2 == 0, a, b).astype(np.uint16)


def solid(W, H, value=9):
    return np.full((H, W), value, np.uint16)


def u_shape(W, H, value=9):
    """Two full columns at the left and right edge joined by the bottom row and --
    a second meeting -- by the top row: a ring, whose halves meet across every
    border between them in two places."""
    d = np.zeros((H, W), np.uint16)
    d[:, 0] = value
    d[:, W - 1] = value
    d[H - 1, :] = value
    d[0, :] = value
    return d


def random_map(W, H, seed, levels=4, invalid=0xFFFF, hi=None):
    """A few disparity levels (so that components of many sizes exist), about 8 %
    `invalid` and 8 % zeros; hi: another 10 % of values up to it."""
    rng = np.random.default_rng(seed)
    d = (10 + rng.integers(0, levels, size=(H, W))).astype(np.uint16)
    if hi:
        big = rng.random((H, W)) < 0.1
        d[big] = rng.integers(hi - 3, hi + 1, size=int(big.sum())).astype(np.uint16)
    d[rng.random((H, W)) < 0.08] = invalid
    d[rng.random((H, W)) < 0.08] = 0
    return d
