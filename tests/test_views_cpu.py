"""tests/views.py on numpy parents: the view builder behind
test_image_views_gpu.py keeps its promises at every base and pitch residue."""
import numpy as np
import pytest

import views

WIDTHS = [1, 9, 70, 203]


def image(W, H=5):
    return np.random.default_rng(W).integers(0, 256, size=(H, W), dtype=np.uint8)


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("base_mod4,pitch_mod4", views.ALL16)
def test_one_view(W, base_mod4, pitch_mod4):
    img = image(W)
    H = img.shape[0]
    parents = {}
    for fill in (0x00, 0xFF, "random"):
        parent, (rect,) = views.build([img], [base_mod4], pitch_mod4, fill, seed=3)
        rows, pitch = parent.shape
        t, l, h, w = rect
        # the residues are the requested ones
        assert pitch == views.pitch_for(W, pitch_mod4) and pitch % 4 == pitch_mod4
        assert (t * pitch + l) % 4 == base_mod4
        # the crop equals the input
        assert (h, w) == (H, W) and np.array_equal(views.crop(parent, rect), img)
        # the margins hold, and [base - 8, base + H * pitch + 8) lies inside the parent
        assert l >= 8 and pitch - W - l >= 8 and t >= 2 and rows - t - H >= 2
        assert t * pitch + l - 8 >= 0 and t * pitch + l + H * pitch + 8 < rows * pitch
        views.check_rect(parent.shape, rect, base_mod4, pitch_mod4)
        parents[fill] = parent
    # two fills differ only outside the view, and there in every byte for 0x00 / 0xFF
    outside = np.ones(parents[0].shape, bool)
    outside[t:t + H, l:l + W] = False
    assert (parents[0x00][outside] == 0x00).all() and (parents[0xFF][outside] == 0xFF).all()
    for a in (0x00, "random"):
        diff = parents[a] != parents[0xFF]
        assert diff.any() and not (diff & ~outside).any()
    assert len(np.unique(parents["random"][outside])) > 16
    views.assert_outside_unchanged(parents[0x00], parents[0x00].copy(), rect)


@pytest.mark.parametrize("pitch_mod4", range(4))
def test_views_of_one_parent_share_the_pitch(pitch_mod4):
    W = 70
    imgs = [image(W, H) for H in (3, 4, 5, 3, 4, 6)]
    mods = [1, 2, 3, 0, 3, 1]
    parent, rects = views.build(imgs, mods, pitch_mod4, "random", seed=1)
    pitch = parent.shape[1]
    assert pitch == views.pitch_for(W, pitch_mod4)
    covered = np.zeros(parent.shape, int)
    for a, b, r in zip(imgs, mods, rects):
        views.check_rect(parent.shape, r, b, pitch_mod4)
        assert np.array_equal(views.crop(parent, r), a)
        covered[r[0] - 1:r[0] + r[2] + 1, :] += 1      # a view and one fill row either side
    assert covered.max() == 1                           # two fill rows between any two views


def test_the_pitch_depends_on_width_and_residue_only():
    for W in WIDTHS:
        for p in range(4):
            got = {views.build([image(W)], [b], p, 0x00)[0].shape[1] for b in range(4)}
            assert got == {views.pitch_for(W, p)}


def test_assert_outside_unchanged_sees_one_byte():
    img = image(9)
    parent, (rect,) = views.build([img], [3], 1, "random")
    t, l, h, w = rect
    inside = parent.copy()
    inside[t:t + h, l:l + w] ^= 0xFF
    views.assert_outside_unchanged(inside, parent, rect)         # the view itself may change
    for y, x in ((t - 1, l), (t, l - 1), (t, l + w), (t + h, l + w - 1), (0, 0),
                 (parent.shape[0] - 1, parent.shape[1] - 1)):
        after = parent.copy()
        after[y, x] ^= 1
        with pytest.raises(AssertionError):
            views.assert_outside_unchanged(after, parent, rect)


def test_the_subset_is_the_fixed_one():
    assert views.SUBSET == [(0, 1), (1, 0), (1, 1), (2, 3), (3, 2), (3, 3)]
    assert len(views.ALL16) == 16 and set(views.SUBSET) <= set(views.ALL16)
