"""The weighted median filter stated on the CPU, independent of
the kernel.

A pixel of a u16 map is valid iff d != invalid and d != 0.  Pixel p is considered
iff (select is None or select[p] != 0) and (fill or p is valid).  Its candidates
are the valid pixels q of the (2r + 1)^2 window inside the frame, p included,
with weight w[|g(p) - g(q)|] > 0 (1 without a guide).  Sorted by (d, qy, qx) the
pick is the first candidate at which twice the running weight reaches the total.
A considered pixel with at least min_support candidates takes the pick's d;
every other pixel keeps its own.

The numpy form stacks the (2r + 1)^2 shifted planes, sorts them by
d * 4096 + window index (the index runs in raster order, so it orders like
(qy, qx)), takes the cumulative weights and the first crossing.  walk() is the
rule pixel by pixel in plain Python, for small frames, to check the numpy form
against."""
import numpy as np

MAX_RADIUS = 15
MAX_SUPPORT = (2 * MAX_RADIUS + 1) ** 2
_ABSENT = np.uint64(0xFFFFFFFF)


def valid(d, invalid):
    return (d != invalid) & (d != 0)


def weights(sigma):
    """The table of sva.wmed_weights: entry i = round(1024 * exp(-i / sigma))."""
    return np.floor(1024.0 * np.exp(-np.arange(256) / float(sigma)) + 0.5).astype(np.uint16)


def _picks_one(d, invalid, r, g, w):
    """(key, n) of one map: per pixel the pick's d * 4096 + window index (junk where
    n = 0) and the number of candidates."""
    H, W = d.shape
    k = 2 * r + 1
    pad = np.zeros((H + 2 * r, W + 2 * r), np.uint16)
    pad[r:r + H, r:r + W] = np.where(valid(d, invalid), d, 0)
    if g is not None:
        gpad = np.zeros(pad.shape, np.int64)
        gpad[r:r + H, r:r + W] = g
        g64 = g.astype(np.int64)
        w64 = np.asarray(w, dtype=np.uint16).astype(np.uint64)
    # one u64 per window cell: (d * 4096 + index) << 17 | weight; absent cells last
    stack = np.empty((k * k, H, W), np.uint64)
    for j in range(k):
        for i in range(k):
            slab = pad[j:j + H, i:i + W].astype(np.uint64)
            wt = (slab != 0).astype(np.uint64)
            if g is not None:
                wt = wt * w64[np.abs(g64 - gpad[j:j + H, i:i + W])]
            idx = j * k + i
            key = np.where(wt > 0, slab * np.uint64(4096) + np.uint64(idx), _ABSENT)
            stack[idx] = (key << np.uint64(17)) | wt
    stack.sort(axis=0)
    wts = (stack & np.uint64(0x1FFFF)).astype(np.int64)
    n = (wts > 0).sum(axis=0)
    cum = np.cumsum(wts, axis=0)
    first = np.argmax(2 * cum >= cum[-1], axis=0)
    key = np.take_along_axis(stack, first[None], axis=0)[0] >> np.uint64(17)
    return key.astype(np.int64), n.astype(np.int64)


def picks(d, invalid, radius, guides=None, weights=None):
    """(key, n), each [..., H, W] i64, of maps d [..., H, W]: what the window of
    every pixel picks, whether or not the pixel is considered.  guides: one [H, W]
    u8 image per map (same leading shape), weights: 256 entries."""
    d = np.asarray(d, dtype=np.uint16)
    assert 1 <= radius <= MAX_RADIUS and (guides is None) == (weights is None)
    H, W = d.shape[-2:]
    flat = d.reshape(-1, H, W)
    g = None if guides is None else np.asarray(guides, dtype=np.uint8).reshape(-1, H, W)
    res = [_picks_one(flat[m], invalid, radius, None if g is None else g[m], weights)
           for m in range(flat.shape[0])]
    return (np.stack([v[0] for v in res]).reshape(d.shape),
            np.stack([v[1] for v in res]).reshape(d.shape))


def apply(d, picked, invalid, radius, subpix=None, select=None, min_support=1, fill=1):
    """(out, out_sub or None, support, written) from picks()'s (key, n)."""
    d = np.asarray(d, dtype=np.uint16)
    assert 1 <= min_support <= MAX_SUPPORT
    key, n = picked
    H, W = d.shape[-2:]
    k = 2 * radius + 1
    look = np.ones(d.shape, bool) if select is None else np.asarray(select).reshape(d.shape) != 0
    if not fill:
        look = look & valid(d, invalid)
    written = look & (n >= min_support) & (n >= 1)
    out = np.where(written, key >> 12, d).astype(np.uint16)
    support = np.where(look, n, 0).astype(np.uint16)
    out_sub = None
    if subpix is not None:
        bits = np.ascontiguousarray(subpix, dtype=np.float32).view(np.uint32).reshape(-1, H, W)
        idx = (key & 4095).reshape(-1, H, W)
        wr = written.reshape(-1, H, W)
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        sy = np.where(wr, yy + idx // k - radius, yy)
        sx = np.where(wr, xx + idx % k - radius, xx)
        m = np.arange(bits.shape[0])[:, None, None]
        out_sub = np.ascontiguousarray(bits[m, sy, sx]).view(np.float32).reshape(d.shape)
    return out, out_sub, support, written


def weighted_median(d, invalid, radius, guides=None, weights=None, subpix=None, select=None,
                    min_support=1, fill=1):
    """(out, out_sub or None, support, written) of maps d [..., H, W]."""
    return apply(d, picks(d, invalid, radius, guides, weights), invalid, radius, subpix, select,
                 min_support, fill)


def walk(d, invalid, radius, guide=None, weights=None, subpix=None, select=None, min_support=1,
         fill=1):
    """weighted_median for ONE small map [H, W], pixel by pixel in plain Python."""
    d = np.asarray(d, dtype=np.uint16)
    H, W = d.shape
    assert H <= 12 and W <= 12
    out = d.copy()
    sub = None if subpix is None else np.array(subpix, dtype=np.float32, copy=True)
    support = np.zeros((H, W), np.uint16)
    written = np.zeros((H, W), bool)
    ok = lambda v: v != invalid and v != 0
    for y in range(H):
        for x in range(W):
            if select is not None and not select[y, x]:
                continue
            if not fill and not ok(int(d[y, x])):
                continue
            cands = []
            for qy in range(max(0, y - radius), min(H, y + radius + 1)):
                for qx in range(max(0, x - radius), min(W, x + radius + 1)):
                    v = int(d[qy, qx])
                    if not ok(v):
                        continue
                    wq = 1 if guide is None else \
                        int(weights[abs(int(guide[y, x]) - int(guide[qy, qx]))])
                    if wq > 0:
                        cands.append((v, qy, qx, wq))
            cands.sort()
            n = len(cands)
            support[y, x] = n
            if n < min_support or n < 1:
                continue
            total = sum(c[3] for c in cands)
            run = 0
            for v, qy, qx, wq in cands:
                run += wq
                if 2 * run >= total:
                    break
            out[y, x] = v
            written[y, x] = True
            if sub is not None:
                sub.view(np.uint32)[y, x] = np.asarray(subpix, np.float32).view(np.uint32)[qy, qx]
    return out, sub, support, written
