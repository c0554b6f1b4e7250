"""Hole filling stated on the CPU, independent of the kernels.

A pixel of a u16 map is valid iff d != invalid and d != 0; every other pixel is a
hole.  Direction k of a hole p looks at p + j * r_k for j = 1..max_dist inside
the frame; the first valid pixel of the input map is its candidate (d, j, k).
The candidates sorted by (d, j, k) -- one integer, d << 11 | j << 3 | k -- `mode`
picks element 0 (MIN), min(1, n - 1) (SECOND) or (n - 1) // 2 (MEDIAN) if there
are at least min_found of them; otherwise, and at valid pixels, nothing changes.

The numpy form takes, per direction and per j, the map shifted by j * r_k and
keeps the first valid value seen: no scan, no carried state.  walk() is the
rule pixel by pixel in plain Python, for small frames, to check the numpy form
against."""
import numpy as np

MIN, SECOND, MEDIAN = 0, 1, 2
MODES = (MIN, SECOND, MEDIAN)
# k: E W S N SE NW SW NE, as (dx, dy)
DIRS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (-1, 1), (1, -1))
ABSENT = 0xFFFFFFFF
MAX_DIST = 255


def valid(d, invalid):
    return (d != invalid) & (d != 0)


def candidates(d, invalid, max_dist):
    """keys [8, ..., H, W] u32 of maps d [..., H, W]: direction k's candidate key
    at every pixel (valid ones too), ABSENT where it has none."""
    d = np.asarray(d, dtype=np.uint16)
    H, W = d.shape[-2:]
    ok = valid(d, invalid)
    wide = d.astype(np.uint32)
    keys = np.full((8,) + d.shape, ABSENT, np.uint32)
    for k, (dx, dy) in enumerate(DIRS):
        for j in range(1, max_dist + 1):
            ox, oy = j * dx, j * dy
            if abs(ox) >= W or abs(oy) >= H:
                break
            ys = slice(max(0, -oy), H - max(0, oy))
            xs = slice(max(0, -ox), W - max(0, ox))
            sys_ = slice(ys.start + oy, ys.stop + oy)
            sxs = slice(xs.start + ox, xs.stop + ox)
            dst = keys[k][..., ys, xs]
            take = ok[..., sys_, sxs] & (dst == ABSENT)
            dst[take] = (wide[..., sys_, sxs][take] << 11) | (j << 3) | k
    return keys


def pick_index(n, mode):
    """The element of the sorted candidates that `mode` picks among n >= 1."""
    if mode == MIN:
        return np.zeros_like(n)
    if mode == SECOND:
        return np.minimum(1, n - 1)
    return (n - 1) // 2


def apply(d, keys, invalid, min_found, mode, subpix=None):
    """(out, out_sub or None, n_found, filled) from candidates()'s keys."""
    d = np.asarray(d, dtype=np.uint16)
    H, W = d.shape[-2:]
    hole = ~valid(d, invalid)
    srt = np.sort(keys, axis=0)
    n = (keys != ABSENT).sum(axis=0)
    idx = pick_index(np.maximum(n, 1), mode)
    chosen = np.take_along_axis(srt, idx[None], axis=0)[0]
    filled = hole & (n >= min_found) & (n >= 1)
    out = np.where(filled, chosen >> 11, d).astype(np.uint16)
    n_found = np.where(hole, n, 0).astype(np.uint8)
    out_sub = None
    if subpix is not None:
        bits = np.ascontiguousarray(subpix, dtype=np.float32).view(np.uint32)
        j = ((chosen >> 3) & 255).astype(np.int64)
        k = (chosen & 7).astype(np.int64)
        dxs = np.array([v[0] for v in DIRS])
        dys = np.array([v[1] for v in DIRS])
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        sy = np.where(filled, yy + j * dys[k], yy)
        sx = np.where(filled, xx + j * dxs[k], xx)
        flat = bits.reshape(-1, H, W)
        m = np.arange(flat.shape[0])[:, None, None]
        got = flat[m, sy.reshape(-1, H, W), sx.reshape(-1, H, W)].reshape(d.shape)
        out_sub = got.view(np.float32)
    return out, out_sub, n_found, filled


def fill_holes(d, invalid, max_dist, min_found=1, mode=SECOND, subpix=None):
    """(out, out_sub or None, n_found, filled) of maps d [..., H, W]."""
    return apply(d, candidates(d, invalid, max_dist), invalid, min_found, mode, subpix)


def walk(d, invalid, max_dist, min_found=1, mode=SECOND, subpix=None):
    """fill_holes for ONE small map [H, W], ray by ray in plain Python."""
    d = np.asarray(d, dtype=np.uint16)
    H, W = d.shape
    assert H <= 12 and W <= 12
    out = d.copy()
    sub = None if subpix is None else np.array(subpix, dtype=np.float32, copy=True)
    n_found = np.zeros((H, W), np.uint8)
    filled = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            if int(d[y, x]) != invalid and int(d[y, x]) != 0:
                continue
            cands = []
            for k, (dx, dy) in enumerate(DIRS):
                for j in range(1, max_dist + 1):
                    qx, qy = x + j * dx, y + j * dy
                    if not (0 <= qx < W and 0 <= qy < H):
                        break
                    v = int(d[qy, qx])
                    if v != invalid and v != 0:
                        cands.append((v, j, k, qy, qx))
                        break
            cands.sort()
            n = len(cands)
            n_found[y, x] = n
            if n >= min_found and n >= 1:
                e = {MIN: 0, SECOND: min(1, n - 1), MEDIAN: (n - 1) // 2}[mode]
                out[y, x] = cands[e][0]
                filled[y, x] = True
                if sub is not None:
                    sub.view(np.uint32)[y, x] = np.asarray(subpix, np.float32).view(np.uint32)[
                        cands[e][3], cands[e][4]]
    return out, sub, n_found, filled


def random_map(W, H, seed, holes=0.3, invalid=0xFFFF, hi=40):
    """[H, W] u16: values 1..hi, a share `holes` of the pixels 0 or `invalid`."""
    rng = np.random.default_rng(seed)
    d = rng.integers(1, hi + 1, (H, W)).astype(np.uint16)
    if invalid != 0:
        d[d == invalid] = 1
    gone = rng.random((H, W)) < holes
    d[gone] = np.where(rng.random((H, W)) < 0.5, invalid, 0)[gone].astype(np.uint16)
    return d


def subpix_of(d, seed=0):
    """f32 planes of distinct values with a few NaN of their own."""
    rng = np.random.default_rng(seed)
    s = (d.astype(np.float32) + rng.random(d.shape, dtype=np.float32) - 0.5).astype(np.float32)
    s[rng.random(d.shape) < 0.03] = np.nan
    return s
