"""Image views for the device-view tests: an H x W u8 image placed inside a
larger parent allocation, as a caller's crop of a bigger image is
(base = parent + y0 * pitch + x0, the parent's pitch), with the residues of
the base address and of the pitch modulo 4 chosen by the test and every parent
byte outside the view set to a known fill.  No fixtures, no GPU calls of its
own (make_view only uploads the parent).

Layout of one parent: rows of `pitch` bytes; TOP rows of fill, then the views
one below the other with GAP rows of fill between them, then at least BOTTOM
rows of fill.  pitch = W + 19 + (0..3), so that every view can take a left
margin of 8..11 bytes -- whichever puts its base on the residue asked for --
and still keeps a right margin of at least 8.  Every byte of
[base - 8, base + H * pitch + 8) of every view therefore lies inside the
parent, and no view ends at the parent's last byte."""
import numpy as np

TOP = 2          # rows of fill above the first view
GAP = 2          # rows of fill between two views of one parent
BOTTOM = 2       # rows of fill below the last view
MARGIN = 8       # least number of fill bytes left and right of a view's rows

ALL16 = [(b, p) for b in range(4) for p in range(4)]
# the fixed subset for cases whose oracle is slow
SUBSET = [(0, 1), (1, 0), (1, 1), (2, 3), (3, 2), (3, 3)]
FILLS = (0x00, 0xFF)


def pitch_for(W, pitch_mod4):
    """The parent pitch of views W wide: the smallest value >= W + 19 on the
    residue asked for (left <= 11 and right >= 8 for every base residue)."""
    return W + MARGIN + 3 + MARGIN + ((pitch_mod4 - (W + MARGIN + 3 + MARGIN)) % 4)


def fill_bytes(shape, fill, seed=0):
    """The parent before the views are written: 0x00, 0xFF or "random"."""
    if isinstance(fill, str):
        assert fill == "random"
        return np.random.default_rng(90000 + seed).integers(0, 256, size=shape, dtype=np.uint8)
    assert fill in (0x00, 0xFF)
    return np.full(shape, fill, np.uint8)


def build(imgs, base_mods, pitch_mod4, fill, seed=0):
    """(parent [rows][pitch] u8, rects): the views of `imgs` (equal widths) in
    one parent whose own base is taken as 4-byte aligned.  rects[i] = (top,
    left, H, W) of view i; its byte offset top * pitch + left has the residue
    base_mods[i] modulo 4."""
    imgs = [np.asarray(a) for a in imgs]
    W = imgs[0].shape[1]
    assert len(imgs) == len(base_mods) and W >= 1
    assert all(a.ndim == 2 and a.dtype == np.uint8 and a.shape[1] == W for a in imgs)
    pitch = pitch_for(W, pitch_mod4)
    rects, top = [], TOP
    for a, b in zip(imgs, base_mods):
        left = MARGIN + ((b - top * pitch - MARGIN) % 4)
        rects.append((top, left, a.shape[0], W))
        top += a.shape[0] + GAP
    parent = fill_bytes((top - GAP + BOTTOM, pitch), fill, seed)
    for a, (t, l, h, w) in zip(imgs, rects):
        parent[t:t + h, l:l + w] = a
    return parent, rects


def check_rect(parent_shape, rect, base_mod4=None, pitch_mod4=None):
    """The promises of this module for one view, asserted."""
    rows, pitch = parent_shape
    t, l, h, w = rect
    assert l >= MARGIN and pitch - w - l >= MARGIN
    assert t >= TOP and rows - (t + h) >= BOTTOM
    off = t * pitch + l
    assert off - 8 >= 0 and off + h * pitch + 8 < rows * pitch
    if base_mod4 is not None:
        assert off % 4 == base_mod4
    if pitch_mod4 is not None:
        assert pitch % 4 == pitch_mod4


def crop(parent, rect):
    t, l, h, w = rect
    return parent[t:t + h, l:l + w]


def _upload(parent, torch_dev):
    import torch
    t = torch.from_numpy(parent).to(torch_dev)
    assert t.data_ptr() % 4 == 0
    return t


def make_views(imgs, base_mods, pitch_mod4, fill, torch_dev, seed=0):
    """Several views in ONE device parent: (parent_tensor, [ptr], pitch)."""
    parent, rects = build(imgs, base_mods, pitch_mod4, fill, seed)
    for r, b in zip(rects, base_mods):
        check_rect(parent.shape, r, b, pitch_mod4)
    t = _upload(parent, torch_dev)
    pitch = parent.shape[1]
    ptrs = [t.data_ptr() + r[0] * pitch + r[1] for r in rects]
    assert all(p % 4 == b for p, b in zip(ptrs, base_mods))
    return t, ptrs, pitch


def make_view(img, base_mod4, pitch_mod4, fill, torch_dev, seed=0):
    """One view in a device parent of its own: (parent_tensor, ptr, pitch),
    ptr % 4 == base_mod4 and pitch % 4 == pitch_mod4; the pitch depends only on
    the width and pitch_mod4, so the views of one call share it."""
    t, ptrs, pitch = make_views([img], [base_mod4], pitch_mod4, fill, torch_dev, seed)
    return t, ptrs[0], pitch


def rect_of(parent_tensor, ptr, pitch, H, W):
    """(top, left, H, W) of the view at device address ptr."""
    off = ptr - parent_tensor.data_ptr()
    return off // pitch, off % pitch, H, W


def assert_outside_unchanged(parent_after, parent_before, view_rect):
    """For outputs that carry a pitch: every parent byte outside the view's
    H x W rectangle keeps its value (both parents as [rows][pitch] arrays)."""
    after, before = np.asarray(parent_after), np.asarray(parent_before)
    assert after.shape == before.shape and after.dtype == before.dtype == np.uint8
    t, l, h, w = view_rect
    outside = np.ones(after.shape, bool)
    outside[t:t + h, l:l + w] = False
    bad = outside & (after != before)
    assert not bad.any(), f"{int(bad.sum())} bytes outside the view changed, first at " \
                          f"{tuple(int(v) for v in np.argwhere(bad)[0])}"
