"""Frames of different kind and size back to back through one engine (DESIGN.md
§7): the post-filter chain moves the maps step 4 reads between the gathered maps,
the check's planes and the median's planes, and regrows its workspaces between
frames.  One engine runs

1. sva_array_depth_smoothed on the banded scene of tests/wmed_scene.py (128 x 96,
   D 32, nine groups): SVA_ARRAY_GROUPS, check 1, sub 1, wmed_select 1, every
   plane the group route returns asked for;
2. sva_array_depth_filtered on SVA_ARRAY_PAIRS, check 0, sub 0, on the same views
   cropped to their top-left 96 x 64, maps and comp_size asked for -- no check and
   no median, so step 4 reads the gathered maps again;
3. the first frame again.

Every plane each frame returns must equal, byte for byte, that of the same call
on an engine that has run nothing else."""
import numpy as np
import pytest

import wmed_expect as we
import wmed_scene as ws

pytestmark = pytest.mark.gpu

CROP_W, CROP_H = 96, 64


def smoothed_frame(m, sva):
    jobs, gs = ws.jobs(sva)
    return m.array_depth_smoothed(
        ws.views(), jobs, gs, ws.F, ws.PS, 5, we.weights(32), 1, 1, fill_max_dist=16,
        fill_min_found=3, fill_mode=sva.SVA_FILL_MEDIAN, speckle_max_size=20, speckle_max_diff=1,
        check=1, view_step=ws.VIEW_STEP, route=sva.SVA_ARRAY_GROUPS, mode=sva.SVA_FUSE_MEDIAN,
        sub=1, want_sub=True, want_maps=True, want_costs=True, want_counts=True, want_size=True,
        want_found=True, want_support=True, **ws.CHECK)


def filtered_frame(m, sva):
    """Two groups of pairs: camera 4 against its eight neighbours, camera 0 against
    its three."""
    jobs, gs = ws.jobs(sva)
    mine = jobs[gs[4]:gs[5]] + jobs[gs[0]:gs[1]]
    views = [np.ascontiguousarray(v[:CROP_H, :CROP_W]) for v in ws.views()]
    return m.array_depth_filtered(
        views, mine, [0, gs[5] - gs[4], gs[5] - gs[4] + gs[1] - gs[0]], ws.F, ws.PS, 20, 1,
        check=0, route=sva.SVA_ARRAY_PAIRS, mode=sva.SVA_FUSE_MEDIAN, sub=0, want_maps=True,
        want_size=True)


def alone(sva, frame):
    m = sva.Multi([0])
    try:
        return frame(m, sva)
    finally:
        m.close()


def assert_same(got, ref, which):
    assert got.keys() == ref.keys()
    for k in ref:
        if ref[k] is None:
            assert got[k] is None, (which, k)
        else:
            assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, (which, k)
            assert got[k].tobytes() == ref[k].tobytes(), (which, k)


def test_three_frames_through_one_engine(sva):
    ref_smoothed, ref_filtered = alone(sva, smoothed_frame), alone(sva, filtered_frame)
    # the frames differ in what they return and are not empty
    for k in ("depth", "subpix", "maps", "cost_min", "cost_second", "agree", "conflict",
              "comp_size", "n_found", "support"):
        assert ref_smoothed[k] is not None, k
    for k in ("depth", "maps", "agree", "comp_size", "n_found", "support"):
        assert ref_smoothed[k].any(), k
    assert ref_smoothed["maps"].shape == (9, ws.H, ws.W)
    assert ref_filtered["maps"].shape == (11, CROP_H, CROP_W)
    assert ref_filtered["depth"].shape == (2, CROP_H, CROP_W)
    assert ref_filtered["comp_size"].any() and ref_filtered["subpix"] is None
    m = sva.Multi([0])
    try:
        first = smoothed_frame(m, sva)
        second = filtered_frame(m, sva)
        third = smoothed_frame(m, sva)
    finally:
        m.close()
    assert_same(first, ref_smoothed, "first")
    assert_same(second, ref_filtered, "second")
    assert_same(third, ref_smoothed, "third")
