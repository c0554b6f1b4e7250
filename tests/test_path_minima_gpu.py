"""Path minima vs the oracle: on the frame route of native
D = 128 (tune::kPathMinima8) the horizontal and vertical lines of sgm_paths
store every pixel's entering minimum, 8 bytes per 8-pixel segment, and the
four recurrences of wta_hv read m from those planes instead of reducing the
state.  A wrong or misplaced byte changes L of every later pixel of its
segment, so the maps are compared with the CPU oracle: disparity bit-equal,
sub-pixel within 1e-5.

Shapes sit around the 16 x 8 tile and the 8-pixel segment: the segment that
gets no checkpoint (the last of directions 0 and 2) must still be flushed, a
ragged segment ends a forward walk (W or H not a multiple of 8) and starts a
backward one.  Both diagonal routes carry the minima; SVA_DEBUG_DIAG_ROUTE
tells which one a frame took, so no case runs the other by accident.  The
stage entry points (sva_paths_tile_d + sva_wta_hv_d) pass no plane and keep
the instances that form m themselves: one test compares the two byte for byte.
"""
import functools

import numpy as np
import pytest
import torch

from stereovisionarray_amd import synth

pytestmark = pytest.mark.gpu

PAIR, FOUR = 1, 0
ROUTES = [PAIR, FOUR]
# (W, H)
SHAPES = [(16, 8), (8, 8), (17, 9), (7, 5), (1, 9), (9, 1), (24, 16), (33, 17), (40, 25), (65, 49)]
# the D class with the minima enabled, native and padded
DS = [128, 100]
PENALTIES = [(10, 120), (1, 127), (0, 0)]
SUB_TOL = 1e-5


@functools.lru_cache(maxsize=None)
def images(W, H):
    L = synth.texture(H, W, W * 11 + H)
    R = synth.texture(H, W, W * 11 + H + 1)
    L.setflags(write=False)
    R.setflags(write=False)
    return L, R


@functools.lru_cache(maxsize=None)
def reference(W, H, D, P1, P2, dmin, dir):
    """The oracle's maps, computed once per frame and shared by both routes."""
    import pyoracle
    L, R = images(W, H)
    od, osub = pyoracle.sgm(L, R, D, dmin, dir, P1, P2, subpixel=True, threads=4)
    od.setflags(write=False)
    osub.setflags(write=False)
    return od, osub


def set_route(ctx, sva, route):
    # every size on the pair route, or none (a threshold no frame reaches)
    ctx.set_debug(sva.SVA_DEBUG_DIAG_PAIR_MIN_PIXELS, 0 if route == PAIR else 1 << 40)


@pytest.fixture(autouse=True)
def default_threshold_after(ctx, sva):
    yield
    ctx.set_debug(sva.SVA_DEBUG_DIAG_PAIR_MIN_PIXELS, -1)


def run(ctx, sva, W, H, D, route, P1=10, P2=120, dmin=0, dir=-1):
    L, R = images(W, H)
    set_route(ctx, sva, route)
    p = sva.default_params(D=D, dmin=dmin, dir=dir, P1=P1, P2=P2, subpixel=1)
    disp, sub = ctx.disparity_sgm(L, R, p)
    assert ctx.get_debug(sva.SVA_DEBUG_DIAG_ROUTE) == route
    return disp, sub


def check(ctx, sva, W, H, D, route, P1=10, P2=120, dmin=0, dir=-1):
    disp, sub = run(ctx, sva, W, H, D, route, P1, P2, dmin, dir)
    od, osub = reference(W, H, D, P1, P2, dmin, dir)
    assert np.array_equal(disp, od), f"{int((disp != od).sum())} pixels differ"
    assert np.max(np.abs(sub - osub)) <= SUB_TOL


@pytest.mark.parametrize("P1,P2", PENALTIES)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("W,H", SHAPES)
def test_shapes(ctx, sva, W, H, D, route, P1, P2):
    check(ctx, sva, W, H, D, route, P1=P1, P2=P2)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("W,H", SHAPES)
def test_dmin_and_dir(ctx, sva, W, H, D, route):
    check(ctx, sva, W, H, D, route, dmin=7, dir=1)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("D", DS)
def test_three_runs_one_context(ctx, sva, D, route):
    """The planes are rewritten by every frame: three runs of one frame on
    one context (with another shape's frame in between, which leaves other
    bytes in the same allocation) give byte-identical maps."""
    W, H = 65, 49
    first = run(ctx, sva, W, H, D, route)
    run(ctx, sva, 33, 17, D, route)
    for _ in range(2):
        again = run(ctx, sva, W, H, D, route)
        assert first[0].tobytes() == again[0].tobytes()
        assert first[1].tobytes() == again[1].tobytes()
    od, osub = reference(W, H, D, 10, 120, 0, -1)
    assert np.array_equal(first[0], od)
    assert np.max(np.abs(first[1] - osub)) <= SUB_TOL


def stage_maps(ctx, sva, torch_dev, L, R, p):
    """The frame through the stage entry points, as tests/test_tile_stages_gpu.py
    drives them: census + cost, sva_paths_tile_d, sva_wta_hv_d."""
    H, W = L.shape
    D = p.D
    lay = sva.tile_layout(W, H, D)
    dL = torch.from_numpy(L.copy()).to(torch_dev)
    dR = torch.from_numpy(R.copy()).to(torch_dev)
    C = torch.zeros((H, W, D), dtype=torch.uint8, device=torch_dev)
    ctx.census_cost_d(dL.data_ptr(), dR.data_ptr(), W, H, W, p, C.data_ptr())
    diag = torch.full((4, H, W, D), 0xAB, dtype=torch.uint8, device=torch_dev)
    hck = torch.full((2, H, lay.nsx, D), 0xCD, dtype=torch.uint8, device=torch_dev)
    vck = torch.full((2, lay.nsy, W, D), 0xEF, dtype=torch.uint8, device=torch_dev)
    assert diag.numel() == lay.diag_bytes and hck.numel() == lay.hckpt_bytes
    assert vck.numel() == lay.vckpt_bytes and C.numel() == lay.cost_bytes
    ctx.paths_tile_d(C.data_ptr(), C.numel(), W, H, p, diag.data_ptr(), diag.numel(),
                     hck.data_ptr(), hck.numel(), vck.data_ptr(), vck.numel())
    disp = torch.zeros((H, W), dtype=torch.int16, device=torch_dev)
    sub = torch.zeros((H, W), dtype=torch.float32, device=torch_dev)
    ctx.wta_hv_d(C.data_ptr(), C.numel(), diag.data_ptr(), diag.numel(), hck.data_ptr(),
                 hck.numel(), vck.data_ptr(), vck.numel(), W, H, p, disp.data_ptr(), sub.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    return disp.cpu().numpy().view(np.uint16), sub.cpu().numpy()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("W,H", [(65, 49), (40, 25), (7, 5)])
def test_frame_matches_stage_entries(ctx, sva, torch_dev, W, H, route):
    """The frame (minima instances) and the stage entry points (the instances
    that form every m themselves), same images: identical bytes."""
    D = 128
    disp, sub = run(ctx, sva, W, H, D, route)
    L, R = images(W, H)
    p = sva.default_params(D=D, dmin=0, dir=-1, P1=10, P2=120, subpixel=1)
    sd, ssub = stage_maps(ctx, sva, torch_dev, L, R, p)
    assert disp.tobytes() == sd.tobytes()
    assert sub.tobytes() == ssub.tobytes()
    od, osub = reference(W, H, D, 10, 120, 0, -1)
    assert np.array_equal(sd, od)
    assert np.max(np.abs(ssub - osub)) <= SUB_TOL
