"""The oracle and the kernels against fixtures made by the reference's own code.

tests/golden/ref_* are the outputs of the reference's Camera.cpp,
functions.cpp and CameraStereoVision.cpp, compiled unmodified against
oracle/cvstandin and driven by oracle/refgen.cpp (tests/golden/
make_ref_golden.py).  Nothing here is compared with the oracle's
own opinion of itself: the CPU tests hold liboracle.so to the fixtures, the GPU
tests hold the kernels to the same fixtures directly.

Every comparison is exact: integers equal, f64 equal as uint64 bit patterns.
Whole arrays are compared against the run in which new Mat storage was zero
(DESIGN.md §2.7's convention); each fixture's `defined*` mask says where that
output is the reference's own behaviour (the positions a second run with fill
0xA5 left unchanged)."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, GOLDEN)
import make_ref_golden as mk  # noqa: E402  (inputs, case tables, packing)

from stereovisionarray_amd import synth  # noqa: E402

_cache = {}


def fx(name):
    if name not in _cache:
        _cache[name] = mk.load(name)
    return _cache[name]


def once(fn):
    """Inputs are regenerated from seeds once per session and shared."""
    key = ("in", fn.__name__)

    def get(*a):
        if key + a not in _cache:
            _cache[key + a] = fn(*a)
        return _cache[key + a]
    return get


in_main, in_shift, in_improve = once(mk.in_main), once(mk.in_shift), once(mk.in_improve)
in_improve_threw, in_shift2 = once(mk.in_improve_threw), once(mk.in_shift2)
in_points, in_depth, in_camera = once(mk.in_points), once(mk.in_depth), once(mk.in_camera)


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rig(make, W):
    return [make(*c) for c in synth.reference_array(0.036 / W)]


def baseline(W, a, b):
    """norm(pos[a] - pos[b]) as the reference evaluates it (CameraStereoVision.cpp:47)."""
    pa, pb = synth.reference_array(0.036 / W)[a][1], synth.reference_array(0.036 / W)[b][1]
    d = [pa[i] - pb[i] for i in range(3)]
    return math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])


IMPROVE_CASES = [(a, b, w) for a, b in mk.IMPROVE_PAIRS for w in mk.IMPROVE_WINDOWS]


# ===================================================================== CPU ==
def test_bresenham_matches_reference(oracle):
    f = fx("ref_bresenham")
    off = f["offsets"]
    pairs = mk.in_bresenham()
    assert len(off) == len(pairs) + 1 and len(pairs) >= 200
    for i, (x0, y0, x1, y1) in enumerate(pairs.tolist()):
        got = oracle.bresenham((x0, y0), (x1, y1))
        assert got == [tuple(p) for p in f["points"][off[i]:off[i + 1]].tolist()], pairs[i]


def test_project_matches_reference(oracle):
    f = fx("ref_camera")
    _, pts = in_camera()
    cams = rig(oracle.OCamera.make, mk.MAIN_W)
    got = np.array([[oracle.project(c, p) for p in pts.tolist()] for c in cams], np.int32)
    assert np.array_equal(got, f["project"])


def test_inv_project_matches_reference(oracle):
    f = fx("ref_camera")
    pix, _ = in_camera()
    cams = rig(oracle.OCamera.make, mk.MAIN_W)
    got = np.array([[oracle.inv_project(c, u, v) for u, v in pix.tolist()] for c in cams])
    assert np.array_equal(u64(got), f["inv_project"])


def test_main_disparity_matches_reference(oracle):
    """The reference's unmodified main() on 25 views (pair 12 -> 11, k = 20)."""
    f = fx("ref_main_160x96")
    views, mask = in_main()
    W, H, k = mk.MAIN_W, mk.MAIN_H, mk.MAIN_K
    cams = rig(oracle.OCamera.make, W)
    d8, _, valid, _ = oracle.ref_pair(views[12], views[11], cams[12], cams[11], k=k, mask=mask)
    written = mk.unpack(f["defined_disparity"], (H, W))
    assert np.array_equal(valid.astype(bool), written)
    assert np.array_equal(d8, f["disparity"])
    # the pixels main() wrote are the masked interior pixels whose endpoints pass
    for y in range(H):
        for x in range(W):
            inside = k <= x < W - k and k <= y < H - k and mask[y, x]
            ok = inside and oracle.ref_endpoints(cams[12], cams[11], W, H, k, 0.5, 1.0, x, y)[0]
            assert bool(ok) == bool(written[y, x]), (x, y)
    # the three bands of the input moved by 12, 16 and 20 px: the matcher must see them
    assert {12, 16, 20} <= set(np.unique(f["disparity"][written]).tolist())


def test_main_depth_matches_reference(oracle):
    f = fx("ref_main_160x96")
    W = mk.MAIN_W
    got = oracle.disp_to_depth(f["disparity"], baseline(W, 12, 11), 0.05, 0.036 / W)
    assert np.array_equal(u64(got), f["depth"])


def test_main_improved_matches_reference(oracle):
    f = fx("ref_main_160x96")
    views, mask = in_main()
    cams = rig(oracle.OCamera.make, mk.MAIN_W)
    st, got = oracle.improve_with_disparity(f["disparity"], views[12], [views[11]],
                                            [(cams[12], cams[11])], window=21, mask=mask,
                                            strict=True)
    assert st == 0
    assert np.array_equal(got, f["improved"])


@pytest.mark.parametrize("b", mk.NEIGHBOURS)
def test_shift_perspective_matches_reference(oracle, b):
    disp, img = in_shift()
    cams = rig(oracle.OCamera.make, mk.SW)
    got = oracle.shift_perspective(cams[12], cams[b], disp, img)
    assert np.array_equal(got, fx("ref_shift_perspective")[f"shifted_{b}"])


@pytest.mark.parametrize("a,b,window", IMPROVE_CASES)
def test_improve_matches_reference(oracle, a, b, window):
    disp, center, img, mask = in_improve(a, b, window)
    cams = rig(oracle.OCamera.make, mk.SW)
    st, got = oracle.improve_with_disparity(disp, center, [img], [(cams[a], cams[b])],
                                            window=window, mask=mask, strict=True)
    exp = fx("ref_shift_improve")[f"improved_{b}_w{window}"]
    assert st == 0
    assert np.array_equal(got, exp)
    if b in (11, 7) and window < 21:   # along the pair's axis the flat patch ties: first minimum
        assert (exp[30:34, 44:52] == disp[30:34, 44:52] - 5).all()


def test_improve_border_window_throws_like_reference(oracle):
    assert fx("ref_shift_improve")["threw_border"].tolist() == [1]
    disp, center, img, mask = in_improve_threw()
    cams = rig(oracle.OCamera.make, mk.SW)
    st, _ = oracle.improve_with_disparity(disp, center, [img], [(cams[12], cams[11])], window=21,
                                          mask=mask, strict=True)
    assert st == -1


@pytest.mark.parametrize("a,b", mk.SHIFT2_PAIRS)
def test_shift_perspective2_matches_reference(oracle, a, b):
    cams = rig(oracle.OCamera.make, mk.SW)
    got = oracle.shift_perspective2(cams[a], cams[b], in_shift2(b))
    assert np.array_equal(u64(got), fx("ref_shift_perspective2")[f"shifted_{b}"])


def test_points_to_depth_matches_reference(oracle):
    cam = rig(oracle.OCamera.make, mk.P2D_W)[12]
    got = oracle.points_to_depth(in_points(), cam, mk.P2D_W, mk.P2D_H)
    assert np.array_equal(u64(got), fx("ref_shift_points_to_depth")["depth"])


def test_depth_to_points_matches_reference(oracle):
    cam = rig(oracle.OCamera.make, mk.D2P_W)[7]
    got = oracle.depth_to_points(in_depth(), cam)
    exp = fx("ref_shift_depth_to_points")["points"]
    assert got.shape == exp.shape
    assert np.array_equal(u64(got), exp)


def _fixtures_present():
    return sorted(n for n in os.listdir(GOLDEN) if n.startswith("ref_"))


def test_fixtures_are_fresh(tmp_path):
    """Re-make every fixture with the reference binary and compare per array."""
    if not os.path.exists(mk.REFGEN):
        # `make` builds the binary exactly when the reference tree (REF_SRC) is there
        import subprocess
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
        if not os.path.exists(mk.REFGEN):
            pytest.skip("no reference binary and no reference tree to build it from")
    mk.write_all(str(tmp_path))
    made = sorted(os.listdir(tmp_path))
    assert made == _fixtures_present()
    for name in made:
        if name.endswith(".json"):
            with open(tmp_path / name) as a, open(os.path.join(GOLDEN, name)) as b:
                assert a.read() == b.read(), name
            continue
        new, old = mk.load(name[:-4], str(tmp_path)), mk.load(name[:-4])
        assert sorted(new) == sorted(old), name
        for k in new:
            assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape, (name, k)
            assert new[k].tobytes() == old[k].tobytes(), (name, k)


def test_fixture_sizes():
    for name in _fixtures_present():
        assert os.path.getsize(os.path.join(GOLDEN, name)) < 64 * 1024, name


# ===================================================================== GPU ==
@pytest.mark.gpu
def test_gpu_main_disparity(ctx, sva):
    f = fx("ref_main_160x96")
    views, mask = in_main()
    cams = rig(sva.Camera.make, mk.MAIN_W)
    d8, d16, valid = ctx.disparity_ref(views[12], views[11], cams[12], cams[11], k=mk.MAIN_K,
                                       mask=mask)
    assert np.array_equal(valid.astype(bool),
                          mk.unpack(f["defined_disparity"], (mk.MAIN_H, mk.MAIN_W)))
    assert np.array_equal(d8, f["disparity"])
    assert np.array_equal(d16, f["disparity"])


@pytest.mark.gpu
def test_gpu_main_depth(ctx, sva):
    f = fx("ref_main_160x96")
    W = mk.MAIN_W
    got = ctx.disparity_to_depth(f["disparity"], baseline(W, 12, 11), 0.05, 0.036 / W)
    assert np.array_equal(u64(got), f["depth"])


@pytest.mark.gpu
def test_gpu_main_improved(ctx, sva):
    f = fx("ref_main_160x96")
    views, mask = in_main()
    cams = rig(sva.Camera.make, mk.MAIN_W)
    got = ctx.improve_with_disparity(f["disparity"], views[12], [views[11]],
                                     [(cams[12], cams[11])], window=21, mask=mask, strict=True)
    assert np.array_equal(got, f["improved"])


@pytest.mark.gpu
@pytest.mark.parametrize("b", mk.NEIGHBOURS)
def test_gpu_shift_perspective(ctx, sva, b):
    disp, img = in_shift()
    cams = rig(sva.Camera.make, mk.SW)
    got = ctx.shift_perspective(cams[12], cams[b], disp, img)
    assert np.array_equal(got, fx("ref_shift_perspective")[f"shifted_{b}"])


def _improve_d(ctx, torch_dev, planes, pair, window, strict):
    """The device entry point on dense planes; returns the output plane."""
    import torch
    disp, center, img, mask = (torch.from_numpy(p).to(torch_dev) for p in planes)
    out = torch.zeros_like(disp)
    ctx.improve_with_disparity_d(disp.data_ptr(), center.data_ptr(), [img.data_ptr()], [pair],
                                 mk.SW, mk.SH, mk.SW, mask.data_ptr(), window, strict,
                                 out.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("a,b,window", IMPROVE_CASES)
def test_gpu_improve(ctx, sva, torch_dev, a, b, window):
    planes = in_improve(a, b, window)
    disp, center, img, mask = planes
    cams = rig(sva.Camera.make, mk.SW)
    exp = fx("ref_shift_improve")[f"improved_{b}_w{window}"]
    got = ctx.improve_with_disparity(disp, center, [img], [(cams[a], cams[b])], window=window,
                                     mask=mask, strict=True)
    assert np.array_equal(got, exp)
    got_d = _improve_d(ctx, torch_dev, planes, (cams[a], cams[b]), window, True)
    assert np.array_equal(got_d, exp)


@pytest.mark.gpu
def test_gpu_improve_border_window_fails_strict(ctx, sva, torch_dev):
    assert fx("ref_shift_improve")["threw_border"].tolist() == [1]
    planes = in_improve_threw()
    disp, center, img, mask = planes
    cams = rig(sva.Camera.make, mk.SW)
    with pytest.raises(sva.SvaError) as e:
        ctx.improve_with_disparity(disp, center, [img], [(cams[12], cams[11])], window=21,
                                   mask=mask, strict=True)
    assert e.value.status == sva.SVA_ERR_INVALID_ARG
    with pytest.raises(sva.SvaError) as e:
        _improve_d(ctx, torch_dev, planes, (cams[12], cams[11]), 21, True)
    assert e.value.status == sva.SVA_ERR_INVALID_ARG


@pytest.mark.gpu
@pytest.mark.parametrize("a,b", mk.SHIFT2_PAIRS)
def test_gpu_shift_perspective2(ctx, sva, a, b):
    cams = rig(sva.Camera.make, mk.SW)
    got = ctx.shift_perspective2(cams[a], cams[b], in_shift2(b))
    assert np.array_equal(u64(got), fx("ref_shift_perspective2")[f"shifted_{b}"])


@pytest.mark.gpu
def test_gpu_points_to_depth(ctx, sva):
    cam = rig(sva.Camera.make, mk.P2D_W)[12]
    got = ctx.points_to_depth(in_points(), cam, mk.P2D_W, mk.P2D_H)
    assert np.array_equal(u64(got), fx("ref_shift_points_to_depth")["depth"])


@pytest.mark.gpu
def test_gpu_depth_to_points(ctx, sva):
    cam = rig(sva.Camera.make, mk.D2P_W)[7]
    got = ctx.depth_to_points(in_depth(), cam)
    exp = fx("ref_shift_depth_to_points")["points"]
    assert got.shape == exp.shape
    assert np.array_equal(u64(got), exp)
