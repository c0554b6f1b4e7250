"""The batched frame route (sva_disparity_sgm_batch_d): n
frames of one shape through one sgm_paths and one wta_hv launch per sub-batch
of tune::kBatchSubFrames frames, whose aggregation overlaps the next
sub-batch's cost kernels on the side streams.  Every
frame's map and sub-pixel map must equal the single-frame route's
(sva_disparity_sgm_d) bit for bit, which the rest of the suite pins to the
oracle; a few frames are checked against the oracle directly.  Frames differ
in their step (1-D and 2-D, both signs), batches run past the 8-frame chunk,
and mismatched parameters are refused."""
import numpy as np
import pytest
import torch

from stereovisionarray_amd import synth

pytestmark = pytest.mark.gpu

STEPS = [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, 1), (-2, -1), (1, -1), (-1, 1)]


def frames(H, W, D, n, seed, steps=STEPS):
    out = []
    for i in range(n):
        sx, sy = steps[i % len(steps)]
        if sy == 0:
            L, R, _ = synth.stereo_pair(H, W, D, 0, sx, seed=seed + i, stripes=4, step=5)
        else:
            L, R, _ = synth.stereo_pair2(H, W, D, 0, sx, sy, seed=seed + i, stripes=4, step=5)
        out.append((L, R, sx, sy))
    return out


def run_batch(ctx, sva, torch_dev, fr, D, subpixel=1, dmin=0):
    H, W = fr[0][0].shape
    dl = [torch.from_numpy(L).to(torch_dev) for L, _, _, _ in fr]
    dr = [torch.from_numpy(R).to(torch_dev) for _, R, _, _ in fr]
    n = len(fr)
    pairs = [(dl[i].data_ptr(), dr[i].data_ptr(),
              sva.default_params(D=D, dmin=dmin, dir=fr[i][2], dir_y=fr[i][3], subpixel=subpixel))
             for i in range(n)]
    maps = torch.full((n, H, W), 0x5A5A, dtype=torch.int16, device=torch_dev)
    sub = torch.zeros((n, H, W), dtype=torch.float32, device=torch_dev)
    ctx.disparity_sgm_batch_d(pairs, W, H, W, maps.data_ptr(), sub.data_ptr())
    one = torch.zeros((H, W), dtype=torch.int16, device=torch_dev)
    one_sub = torch.zeros((H, W), dtype=torch.float32, device=torch_dev)
    ref_m, ref_s = [], []
    for i in range(n):
        ctx.disparity_sgm_d(dl[i].data_ptr(), dr[i].data_ptr(), W, H, W, pairs[i][2],
                            one.data_ptr(), one_sub.data_ptr())
        ctx.synchronize()
        ref_m.append(one.cpu().numpy().copy())
        ref_s.append(one_sub.cpu().numpy().copy())
    ctx.synchronize()
    torch.cuda.synchronize()
    return maps.cpu().numpy(), sub.cpu().numpy(), ref_m, ref_s


@pytest.mark.parametrize("D", [64, 128, 192, 256])
@pytest.mark.parametrize("H,W", [(40, 77), (17, 130), (64, 64)])
def test_batch_equals_single_frames(ctx, sva, torch_dev, D, H, W):
    fr = frames(H, W, D, 5, seed=H * W + D)
    maps, sub, ref_m, ref_s = run_batch(ctx, sva, torch_dev, fr, D)
    for i in range(len(fr)):
        assert np.array_equal(maps[i], ref_m[i]), f"frame {i} step {fr[i][2:]}"
        assert np.array_equal(sub[i].view(np.uint32), ref_s[i].view(np.uint32)), f"sub {i}"


# Steps no census+cost kernel takes -- (1, 3), (4, 1), (-1, 2) -- among fused
# ones: census_pair + cost2 through the side streams' census scratch.
SPLIT_MIX = [(1, 3), (-1, 0), (4, 1), (-1, 2), (1, 3), (0, 1), (4, 1)]


def test_batch_split_route_shares_a_census_slot(ctx, sva, oracle, torch_dev):
    """7 frames over 3 side streams and sub-batches of 4: stream 0 carries
    frames 0, 3 and 6, three split-route frames in a row through one
    census_side slot, across two sub-batches."""
    D, H, W = 64, 40, 77
    fr = frames(H, W, D, 7, seed=H * W + D, steps=SPLIT_MIX)
    maps, sub, ref_m, ref_s = run_batch(ctx, sva, torch_dev, fr, D)
    for i in range(len(fr)):
        assert np.array_equal(maps[i], ref_m[i]), f"frame {i} step {fr[i][2:]}"
        assert np.array_equal(sub[i].view(np.uint32), ref_s[i].view(np.uint32)), f"sub {i}"
    for i in (0, 2, 3):
        L, R, sx, sy = fr[i]
        od, osub = oracle.sgm2(L, R, D, 0, sx, sy, subpixel=True)
        assert np.array_equal(maps[i].view(np.uint16), od), i
        assert np.max(np.abs(sub[i] - osub)) <= 1e-5, i


def test_batch_past_one_chunk_and_padded_D(ctx, sva, torch_dev):
    """11 frames (two launches of 8 + 3), D = 100 (run at 128, padded)."""
    fr = frames(33, 90, 100, 11, seed=5)
    maps, sub, ref_m, ref_s = run_batch(ctx, sva, torch_dev, fr, 100)
    for i in range(len(fr)):
        assert np.array_equal(maps[i], ref_m[i]), i
        assert np.array_equal(sub[i].view(np.uint32), ref_s[i].view(np.uint32)), i


def test_batch_against_oracle(ctx, sva, oracle, torch_dev):
    D, H, W = 64, 30, 110
    fr = frames(H, W, D, 4, seed=9)
    maps, sub, _, _ = run_batch(ctx, sva, torch_dev, fr, D, dmin=2)
    for i, (L, R, sx, sy) in enumerate(fr):
        od, osub = oracle.sgm2(L, R, D, 2, sx, sy, subpixel=True)
        assert np.array_equal(maps[i].view(np.uint16), od), i
        assert np.max(np.abs(sub[i] - osub)) <= 1e-5, i


def test_batch_without_subpixel(ctx, sva, torch_dev):
    fr = frames(20, 50, 64, 3, seed=2)
    maps, sub, ref_m, _ = run_batch(ctx, sva, torch_dev, fr, 64, subpixel=0)
    for i in range(3):
        assert np.array_equal(maps[i], ref_m[i])
    assert (sub == 0).all()


def test_batch_refuses_mixed_params(ctx, sva, torch_dev):
    H, W = 16, 40
    a = torch.zeros((H, W), dtype=torch.uint8, device=torch_dev)
    maps = torch.zeros((2, H, W), dtype=torch.int16, device=torch_dev)
    p0 = sva.default_params(D=64)
    for bad, status in ((sva.default_params(D=128), sva.SVA_ERR_INVALID_ARG),
                        (sva.default_params(D=64, dmin=3), sva.SVA_ERR_INVALID_ARG),
                        (sva.default_params(D=64, P2=100), sva.SVA_ERR_INVALID_ARG),
                        (sva.default_params(D=64, lr_check=1), sva.SVA_ERR_UNSUPPORTED)):
        with pytest.raises(sva.SvaError) as e:
            ctx.disparity_sgm_batch_d([(a.data_ptr(), a.data_ptr(), p0),
                                       (a.data_ptr(), a.data_ptr(), bad)], W, H, W,
                                      maps.data_ptr())
        assert e.value.status == status
    with pytest.raises(sva.SvaError) as e:
        ctx.disparity_sgm_batch_d([], W, H, W, maps.data_ptr())
    assert e.value.status == sva.SVA_ERR_INVALID_ARG


def test_batch_back_to_back_calls(ctx, sva, torch_dev):
    """Two batch calls queued with no synchronisation between them (the second
    call's side-stream cost kernels must not overwrite the first call's cost
    volumes while its sub-batches aggregate), 9 frames each: sub-batches of
    4 + 4 + 1 over three side streams."""
    H, W, D = 36, 70, 64
    fa = frames(H, W, D, 9, seed=31)
    fb = frames(H, W, D, 9, seed=71)
    dev_ = lambda a: torch.from_numpy(a).to(torch_dev)
    calls = []
    for fr in (fa, fb):
        dl = [dev_(L) for L, _, _, _ in fr]
        dr = [dev_(R) for _, R, _, _ in fr]
        pairs = [(dl[i].data_ptr(), dr[i].data_ptr(),
                  sva.default_params(D=D, dir=fr[i][2], dir_y=fr[i][3], subpixel=1))
                 for i in range(len(fr))]
        maps = torch.zeros((len(fr), H, W), dtype=torch.int16, device=torch_dev)
        sub = torch.zeros((len(fr), H, W), dtype=torch.float32, device=torch_dev)
        calls.append((fr, dl, dr, pairs, maps, sub))
    for fr, dl, dr, pairs, maps, sub in calls:          # queued back to back
        ctx.disparity_sgm_batch_d(pairs, W, H, W, maps.data_ptr(), sub.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    one = torch.zeros((H, W), dtype=torch.int16, device=torch_dev)
    one_sub = torch.zeros((H, W), dtype=torch.float32, device=torch_dev)
    for fr, dl, dr, pairs, maps, sub in calls:
        got, gsub = maps.cpu().numpy(), sub.cpu().numpy()
        for i in range(len(fr)):
            ctx.disparity_sgm_d(dl[i].data_ptr(), dr[i].data_ptr(), W, H, W, pairs[i][2],
                                one.data_ptr(), one_sub.data_ptr())
            ctx.synchronize()
            assert np.array_equal(got[i], one.cpu().numpy()), i
            assert np.array_equal(gsub[i].view(np.uint32), one_sub.cpu().numpy().view(np.uint32)), i


def test_batch_failed_cost_launch_joins_side_streams(ctx, sva, torch_dev):
    """a cost launch that fails mid-batch must still leave the
    context stream ordered after every side-stream kernel already queued, so
    the caller may reuse the images and the cost workspace once the context
    stream has drained.  SVA_DEBUG_FAIL_COST_AT fails frame 7 of 9 (frames
    1-6 are queued on the three side streams, big enough to still be running
    when the call returns); after sva_synchronize of the context stream alone,
    every side stream must be idle.  The context then keeps working."""
    H, W, D = 1080, 1920, 128
    fr = frames(H, W, D, 9, seed=91)
    dl = [torch.from_numpy(L).to(torch_dev) for L, _, _, _ in fr]
    dr = [torch.from_numpy(R).to(torch_dev) for _, R, _, _ in fr]
    pairs = [(dl[i].data_ptr(), dr[i].data_ptr(),
              sva.default_params(D=D, dir=fr[i][2], dir_y=fr[i][3], subpixel=1))
             for i in range(len(fr))]
    maps = torch.zeros((len(fr), H, W), dtype=torch.int16, device=torch_dev)
    sub = torch.zeros((len(fr), H, W), dtype=torch.float32, device=torch_dev)
    torch.cuda.synchronize()
    ctx.set_debug(sva.SVA_DEBUG_FAIL_COST_AT, 7)
    with pytest.raises(sva.SvaError) as e:
        ctx.disparity_sgm_batch_d(pairs, W, H, W, maps.data_ptr(), sub.data_ptr())
    assert e.value.status == sva.SVA_ERR_DEVICE
    assert ctx.get_debug(sva.SVA_DEBUG_FAIL_COST_AT) == 0      # one-shot
    ctx.synchronize()                                           # the context stream only
    assert ctx.get_debug(sva.SVA_DEBUG_SIDE_IDLE) == 1
    # the same context and workspaces afterwards: frames 1..3 through the batch
    # route equal the single-frame route
    got, gsub, ref_m, ref_s = run_batch(ctx, sva, torch_dev, fr[:3], D)
    for i in range(3):
        assert np.array_equal(got[i].view(np.uint16), ref_m[i].view(np.uint16)), i
        assert np.array_equal(gsub[i].view(np.uint32), ref_s[i].view(np.uint32)), i


def test_debug_switch_keys(ctx, sva):
    """sva_set_debug / sva_get_debug: range checks, read-only and unknown keys."""
    with pytest.raises(sva.SvaError):
        ctx.set_debug(sva.SVA_DEBUG_PLANE_SPLIT, 17)
    with pytest.raises(sva.SvaError):
        ctx.set_debug(sva.SVA_DEBUG_SIDE_IDLE, 1)
    with pytest.raises(sva.SvaError):
        ctx.get_debug(99)
    ctx.set_debug(sva.SVA_DEBUG_PLANE_SPLIT, 3)
    assert ctx.get_debug(sva.SVA_DEBUG_PLANE_SPLIT) == 3
    ctx.set_debug(sva.SVA_DEBUG_PLANE_SPLIT, 0)
    assert ctx.get_debug(sva.SVA_DEBUG_PLANE_SPLIT) == 0
