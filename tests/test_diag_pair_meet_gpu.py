"""The pair line that meets in the middle vs the oracle: two
16-lane rows of a wave work one diagonal pair, role T the down recurrence over
the rows above the split row M and role B the up recurrence over the rows
below it; each then continues through the other half from the other role's
checkpoints and stores the pair sum E.  The shapes are the ones where the
split can go wrong: two segments, an odd segment count, a ragged last segment,
a wrap at the split row, frames narrower than a wave's rows, line counts
around the 8-line pair block.  Disparity maps bit-equal, sub-pixel within
1e-5, the pair route asserted through SVA_DEBUG_DIAG_ROUTE; the module lowers
the size threshold to 0 and restores it."""
import numpy as np
import pytest

from stereovisionarray_amd import synth

pytestmark = pytest.mark.gpu

PAIR = 1
PAIR_D = [128, 100]

# (W, H); the segment is 8 rows, the split row M = 8 * (ceil(H / 8) // 2)
SIZES = [
    # exactly two segments, two plus a ragged row, a bottom half of one row
    (33, 16), (33, 17), (33, 9),
    # odd segment count, and an odd count with a ragged end
    (40, 24), (40, 25), (21, 43),
    # a wrap exactly at the split row and inside the segments next to it
    (8, 16), (4, 24), (12, 24), (9, 32),
    # W < 4 with several segments
    (1, 33), (2, 20), (3, 26),
    # line counts around the 8-line pair block and the wave's 2-line halves
    (7, 24), (8, 24), (9, 24), (15, 24), (17, 24),
    # a taller narrow frame with many segments per half
    (50, 130),
]


@pytest.fixture(autouse=True)
def pair_at_every_size(ctx, sva):
    ctx.set_debug(sva.SVA_DEBUG_DIAG_PAIR_MIN_PIXELS, 0)
    yield
    ctx.set_debug(sva.SVA_DEBUG_DIAG_PAIR_MIN_PIXELS, -1)


def check(ctx, sva, oracle, L, R, D, dmin=0, dir=-1, P1=10, P2=120):
    p = sva.default_params(D=D, dmin=dmin, dir=dir, P1=P1, P2=P2, subpixel=1)
    disp, sub = ctx.disparity_sgm(L, R, p)
    assert ctx.get_debug(sva.SVA_DEBUG_DIAG_ROUTE) == PAIR
    od, osub = oracle.sgm(L, R, D, dmin, dir, P1, P2, subpixel=True, threads=4)
    assert np.array_equal(disp, od)
    assert np.max(np.abs(sub - osub)) <= 1e-5


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("D", PAIR_D)
def test_split_shapes(ctx, sva, oracle, W, H, D):
    L = synth.texture(H, W, W * 11 + H)
    R = synth.texture(H, W, W * 11 + H + 1)
    check(ctx, sva, oracle, L, R, D)


# the restart and the padded-disparity paths in both roles
@pytest.mark.parametrize("P1,P2", [(1, 127), (0, 0)])
@pytest.mark.parametrize("D", PAIR_D)
def test_penalties(ctx, sva, oracle, D, P1, P2):
    W, H = 40, 25
    L, R, _ = synth.stereo_pair(H, W, D, 0, -1, seed=3)
    check(ctx, sva, oracle, L, R, D, P1=P1, P2=P2)


@pytest.mark.parametrize("D", PAIR_D)
def test_dir_and_dmin(ctx, sva, oracle, D):
    W, H = 40, 25
    L, R, _ = synth.stereo_pair(H, W, D, 7, 1, seed=21)
    check(ctx, sva, oracle, L, R, D, dmin=7, dir=1)


@pytest.mark.parametrize("D", PAIR_D)
def test_repeatable(ctx, sva, D):
    """One frame three times on one context: byte-identical maps (a cheap
    screen for a checkpoint hand-off that is not ordered)."""
    W, H = 65, 49
    L, R, _ = synth.stereo_pair(H, W, D, 0, -1, seed=8)
    p = sva.default_params(D=D, dir=-1, subpixel=1)
    outs = []
    for _ in range(3):
        disp, sub = ctx.disparity_sgm(L, R, p)
        assert ctx.get_debug(sva.SVA_DEBUG_DIAG_ROUTE) == PAIR
        outs.append((disp.tobytes(), sub.tobytes()))
    assert outs[1] == outs[0] and outs[2] == outs[0]
