"""The plan a whole frame runs (frame_plan), stage by stage
through sva_paths_frame_d and sva_wta_frame_d, byte for byte against the CPU
oracle: at native D = 128 the two pair-sum volumes (§4.15, §4.16) with their
row-checkpoint planes and the path-minima planes (§4.17), elsewhere four
volumes without minima; the horizontal and vertical checkpoints by the rules
of test_tile_stages_gpu.py (stage_expect.py); then disp, the sub-pixel map as
bits, cost_min / cost_second and the uniqueness filter, from the plain and the
confidence instance of wta_hv.

Every expected byte is numpy on oracle.path(C, r, P1, P2), r = 0..7, at the
caller's D.  The caller's buffers start poisoned and carry guard bytes behind
the layout's sizes; what the layout calls "not written" must keep its poison.
test_product_equality ties the entries to the product: sva_disparity_sgm_conf
on the same images gives the same four planes bit for bit, on the route the
layout reports.  The module lowers the pair route's pixel threshold to 0 (as
test_diag_pair_gpu.py), so that small frames run the instances 1080p runs."""
import numpy as np
import pytest
import torch

import conf_expect as ce
import stage_expect as se
from stereovisionarray_amd import synth
from test_diag_pair_gpu import SIZES

pytestmark = pytest.mark.gpu

PAIR, FOUR = 1, 0
PAIR_D = [128, 100]        # the D class with the pair route and minima, and a padded D of it
INVALID = 0xFFFF
GUARD = 384                # bytes behind volumes_bytes and ckpt_bytes
POISON = (0xAB, 0xCD)      # volumes, checkpoint buffer
# beyond test_diag_pair_gpu's sizes: more than one block of 16 lines, ragged last segment
MORE_SIZES = [(130, 17), (257, 21)]
FAMILIES = ["image", "uniform", "wells", "const62"]


@pytest.fixture(autouse=True)
def pair_at_every_size(ctx, sva):
    ctx.set_debug(sva.SVA_DEBUG_DIAG_PAIR_MIN_PIXELS, 0)
    yield
    ctx.set_debug(sva.SVA_DEBUG_DIAG_PAIR_MIN_PIXELS, -1)


def cost_volume(oracle, kind, W, H, D, seed):
    """C [H][W][D] u8 within the legal range 0..62."""
    rng = np.random.RandomState(seed)
    if kind == "texture":      # two independent textures, as test_diag_pair_gpu.test_sizes
        L, R = synth.texture(H, W, W * 7 + H), synth.texture(H, W, W * 7 + H + 1)
        return oracle.cost(oracle.census(L), oracle.census(R), D, 0, -1)
    if kind == "image":
        L, R, _ = synth.stereo_pair(H, W, D, 0, -1, seed=seed)
        return oracle.cost(oracle.census(L), oracle.census(R), D, 0, -1)
    if kind == "uniform":
        return rng.randint(0, 63, size=(H, W, D)).astype(np.uint8)
    if kind == "const62":
        return np.full((H, W, D), 62, np.uint8)
    assert kind == "wells"
    C = np.full((H, W, D), 62, np.uint8)
    d0 = rng.randint(0, D, size=((H + 3) // 4, (W + 3) // 4))
    d0 = np.repeat(np.repeat(d0, 4, axis=0), 4, axis=1)[:H, :W]
    np.put_along_axis(C, d0[:, :, None], 0, axis=2)
    flat = rng.rand(H, W) < 0.15
    C[flat] = rng.randint(0, 3, size=(int(flat.sum()), D)).astype(np.uint8)
    return C


_EXPECT = {}


def expect(oracle, kind, W, H, D, P1, P2, seed=3):
    """The oracle's side of a case, computed once and left unchanged."""
    key = (kind, W, H, D, P1, P2, seed)
    if key not in _EXPECT:
        C = cost_volume(oracle, kind, W, H, D, seed)
        assert C.max() <= 62
        vols = se.path_volumes(oracle, C, P1, P2)
        S = se.volume_sum(vols)
        disp, sub = oracle.wta(S, 0, True)
        ds, cmin, csec = ce.conf_planes(S)
        assert np.array_equal(disp, ds.astype(np.uint16))
        e = dict(C=C, vols=vols, S=S, disp=disp, sub=sub, cmin=cmin, csec=csec)
        for v in [C, S, disp, sub, cmin, csec] + vols:
            v.setflags(write=False)
        _EXPECT[key] = e
    return _EXPECT[key]


def dev(a, d):
    return torch.from_numpy(np.ascontiguousarray(a)).to(d)


def host(ctx, t):
    ctx.synchronize()
    torch.cuda.synchronize()
    return t.cpu().numpy()


def native_cost(C, Dn):
    """The caller's C at the native width: 255 at d >= D (§4.7)."""
    H, W, D = C.shape
    Cn = np.full((H, W, Dn), 255, np.uint8)
    Cn[:, :, :D] = C
    return Cn


class Planes:
    """The two caller buffers of a frame plan, poisoned, with guard bytes."""

    def __init__(self, lay, torch_dev):
        self.lay = lay
        self.vol = torch.full((lay.volumes_bytes + GUARD,), POISON[0], dtype=torch.uint8,
                              device=torch_dev)
        self.ck = torch.full((lay.ckpt_bytes + GUARD,), POISON[1], dtype=torch.uint8,
                             device=torch_dev)

    def fetch(self, ctx, W, H):
        lay = self.lay
        v, k = host(ctx, self.vol), host(ctx, self.ck)
        self.raw = (v, k)
        self.guards = (v[lay.volumes_bytes:], k[lay.ckpt_bytes:])
        self.volumes = v[:lay.volumes_bytes].reshape(lay.n_volumes, H, W, lay.D)

        def part(off, nbytes, shape):
            assert off + nbytes <= lay.ckpt_bytes
            return k[off:off + nbytes].reshape(shape)
        self.hck = part(lay.hck_off, lay.hck_bytes, (2, H, lay.nsx, lay.D))
        self.vck = part(lay.vck_off, lay.vck_bytes, (2, lay.nsy, W, lay.D))
        self.pck = part(lay.pair_off, lay.pair_bytes, (2, lay.nsy, W, lay.D)) if lay.route == PAIR else None
        self.hmn = part(lay.hmn_off, lay.hmn_bytes, (2, H, lay.nsx, 8)) if lay.minima else None
        self.vmn = part(lay.vmn_off, lay.vmn_bytes, (2, lay.nsy, W, 8)) if lay.minima else None


def check_layout(lay, W, H, Dn, want):
    """The plane groups tile the checkpoint buffer in §4.9a's order."""
    assert (lay.route, lay.D, lay.seg) == (want, Dn, 8)
    assert lay.minima == (1 if Dn == 128 else 0)
    assert (lay.nsx, lay.nsy) == (-(-W // 8), -(-H // 8))
    assert lay.n_volumes == (2 if want == PAIR else 4)
    assert lay.cost_bytes == W * H * Dn and lay.volumes_bytes == lay.n_volumes * lay.cost_bytes
    assert lay.hck_bytes == 2 * H * lay.nsx * Dn and lay.vck_bytes == 2 * lay.nsy * W * Dn
    assert lay.pair_bytes == (lay.vck_bytes if want == PAIR else 0)
    assert lay.hmn_bytes == (2 * H * lay.nsx * 8 if lay.minima else 0)
    assert lay.vmn_bytes == (2 * lay.nsy * W * 8 if lay.minima else 0)
    off = 0
    for o, n in ((lay.hck_off, lay.hck_bytes), (lay.vck_off, lay.vck_bytes),
                 (lay.pair_off, lay.pair_bytes), (lay.hmn_off, lay.hmn_bytes),
                 (lay.vmn_off, lay.vmn_bytes)):
        assert o == off
        off += n
    assert lay.ckpt_bytes == off


def check_paths(pl, e, D, want):
    """Everything sva_paths_frame_d left in the two buffers."""
    lay, C, vols = pl.lay, e["C"], e["vols"]
    for g, poison in zip(pl.guards, POISON):
        assert g.size == GUARD and (g == poison).all(), "bytes behind the buffer were written"
    if want == PAIR:
        for j, E in enumerate(se.pair_sums(C, vols)):
            bad = pl.volumes[j][:, :, :D] != E
            assert not bad.any(), f"pair sum {j}: {int(bad.sum())} bytes differ, first at {np.argwhere(bad)[0]}"
        se.check_pair_planes(pl.pck, vols, lay.seg, D)
        for s in se.pair_plane_rows(lay.nsy)[2]:
            assert (pl.pck[:, s] == POISON[1]).all(), ("pair plane row written", s)
    else:
        for slot in range(4):
            assert np.array_equal(pl.volumes[slot][:, :, :D], vols[4 + slot]), f"direction {4 + slot}"
    se.check_checkpoints(pl.hck, pl.vck, vols, lay.seg, lay.nsx, lay.nsy, D)
    for part in se.unwritten_checkpoints(pl.hck, pl.vck):
        assert (part == POISON[1]).all(), "a checkpoint entry without a rule was written"
    if lay.minima:
        hmn, vmn, hmask, vmask = se.minima_planes(vols, lay.nsx, lay.nsy)
        for name, got, exp, mask in (("hmn", pl.hmn, hmn, hmask), ("vmn", pl.vmn, vmn, vmask)):
            bad = (got != exp) & mask
            assert not bad.any(), f"{name}: {int(bad.sum())} bytes differ, first at {np.argwhere(bad)[0]}"


def check_outputs(got, e, u):
    disp, sub, cmin, csec = got
    rej = ce.rejected(e["cmin"], e["csec"], u)
    exp_disp, _ = ce.apply_filter(e["disp"], None, rej, INVALID)
    assert np.array_equal(disp, exp_disp), f"disp: {int((disp != exp_disp).sum())} differ (u = {u})"
    assert np.isnan(sub[rej]).all()
    assert np.array_equal(sub.view(np.uint32)[~rej], e["sub"].view(np.uint32)[~rej]), \
        f"sub-pixel bits (u = {u})"
    if cmin is not None:
        assert np.array_equal(cmin, e["cmin"]) and np.array_equal(csec, e["csec"])


def run_wta(ctx, pl, d_C, W, H, p, u, conf, torch_dev):
    """(disp, sub, cost_min, cost_second) of sva_wta_frame_d; conf False: null
    planes (with u = 0 the plain instance)."""
    lay = pl.lay
    disp = torch.zeros((H, W), dtype=torch.int16, device=torch_dev)
    sub = torch.zeros((H, W), dtype=torch.float32, device=torch_dev)
    cmin = torch.zeros((H, W), dtype=torch.int16, device=torch_dev) if conf else None
    csec = torch.zeros((H, W), dtype=torch.int16, device=torch_dev) if conf else None
    ctx.wta_frame_d(d_C.data_ptr(), d_C.numel(), pl.vol.data_ptr(), lay.volumes_bytes,
                    pl.ck.data_ptr(), lay.ckpt_bytes, W, H, p, u, disp.data_ptr(), sub.data_ptr(),
                    cmin.data_ptr() if conf else None, csec.data_ptr() if conf else None)
    return (host(ctx, disp).view(np.uint16), host(ctx, sub),
            host(ctx, cmin).view(np.uint16) if conf else None,
            host(ctx, csec).view(np.uint16) if conf else None)


def run_case(ctx, sva, torch_dev, e, D, P1, P2, want):
    """Both entries on e's cost volume: every plane, then every output."""
    H, W, _ = e["C"].shape
    Dn = ce.padded(D)
    p = sva.default_params(D=D, P1=P1, P2=P2, subpixel=1, invalid=INVALID)
    lay = sva.frame_layout(W, H, p, 0)
    check_layout(lay, W, H, Dn, want)
    d_C = dev(native_cost(e["C"], Dn), torch_dev)
    assert d_C.numel() == lay.cost_bytes
    pl = Planes(lay, torch_dev)
    ctx.paths_frame_d(d_C.data_ptr(), d_C.numel(), W, H, p, pl.vol.data_ptr(), lay.volumes_bytes,
                      pl.ck.data_ptr(), lay.ckpt_bytes)
    pl.fetch(ctx, W, H)
    check_paths(pl, e, D, want)
    before = pl.raw
    check_outputs(run_wta(ctx, pl, d_C, W, H, p, 0, False, torch_dev), e, 0)   # plain instance
    for u in (0, 10):
        check_outputs(run_wta(ctx, pl, d_C, W, H, p, u, True, torch_dev), e, u)
    pl.fetch(ctx, W, H)                # the second stage only reads the two buffers
    assert np.array_equal(pl.raw[0], before[0]) and np.array_equal(pl.raw[1], before[1])
    return pl


@pytest.mark.parametrize("W,H", SIZES + MORE_SIZES)
@pytest.mark.parametrize("D", PAIR_D)
def test_sizes(ctx, sva, oracle, torch_dev, W, H, D):
    e = expect(oracle, "texture", W, H, D, 10, 120)
    run_case(ctx, sva, torch_dev, e, D, 10, 120, PAIR)


def test_sizes_cover_a_wrap_inside_a_segment():
    """Sizes with W < 8 make a pair line cross the image edge inside an 8-row
    segment, the slow path of pair_line's second phase."""
    inside = [(W, H) for W, H in SIZES + MORE_SIZES if se.pair_line_wraps_inside_segment(W, H)]
    assert any(W < 8 for W, H in inside) and any(W >= 16 for W, H in inside)
    assert not se.pair_line_wraps_inside_segment(1, 1)


# 127 is the largest P2 a u8 pair sum carries; (130, 127): P1 > P2
PENALTIES = [(10, 120, PAIR), (0, 0, PAIR), (1, 127, PAIR), (130, 127, PAIR), (10, 128, FOUR),
             (193, 193, FOUR)]


@pytest.mark.parametrize("P1,P2,want", PENALTIES)
@pytest.mark.parametrize("D", PAIR_D)
def test_penalties(ctx, sva, oracle, torch_dev, D, P1, P2, want):
    e = expect(oracle, "image", 65, 31, D, P1, P2)
    if (P1, P2) == (193, 193):
        assert any((v == 255).any() for v in e["vols"])      # the u8 paths saturate
    run_case(ctx, sva, torch_dev, e, D, P1, P2, want)


@pytest.mark.parametrize("D", [64, 192, 256])
def test_other_d_run_four_volumes_without_minima(ctx, sva, oracle, torch_dev, D):
    e = expect(oracle, "image", 65, 31, D, 10, 120)
    pl = run_case(ctx, sva, torch_dev, e, D, 10, 120, FOUR)
    assert pl.lay.minima == 0 and pl.lay.ckpt_bytes == pl.lay.hck_bytes + pl.lay.vck_bytes


@pytest.mark.parametrize("P1,P2", [(10, 120), (1, 127)])
@pytest.mark.parametrize("kind", FAMILIES)
def test_cost_families(ctx, sva, oracle, torch_dev, kind, P1, P2):
    """Volumes only a caller's C can supply, beside the image-derived one: the
    pair sums reach 2 * P2 (the u8's last carry-free value at P2 = 127), and
    the minima planes span the legal range."""
    W, H, D = 65, 31, 128
    e = expect(oracle, kind, W, H, D, P1, P2)
    E = se.pair_sums(e["C"], e["vols"])
    if kind != "const62":
        assert any((x == 2 * P2).any() for x in E), "no pair sum at 2 * P2"
    if kind in ("image", "wells"):
        hmn, vmn, hmask, vmask = se.minima_planes(e["vols"], -(-W // 8), -(-H // 8))
        mn = np.concatenate([hmn[hmask], vmn[vmask]])
        assert (mn == 0).any() and (mn == 62).any()
    run_case(ctx, sva, torch_dev, e, D, P1, P2, PAIR)


def test_product_equality(ctx, sva, oracle, torch_dev):
    """sva_disparity_sgm_conf on images against sva_census_cost_d + the two
    entries: four planes bit for bit, on the route the layout reports, with
    the pixel threshold at 0, at W * H and at W * H + 1."""
    W, H, D = 65, 31, 128
    L, R, _ = synth.stereo_pair(H, W, D, 0, -1, seed=3)
    p = sva.default_params(D=D, subpixel=1, invalid=INVALID)
    dL, dR = dev(L, torch_dev), dev(R, torch_dev)
    d_C = torch.zeros((H, W, D), dtype=torch.uint8, device=torch_dev)
    ctx.census_cost_d(dL.data_ptr(), dR.data_ptr(), W, H, W, p, d_C.data_ptr())
    e = expect(oracle, "image", W, H, D, 10, 120)
    assert np.array_equal(host(ctx, d_C), e["C"])
    for thr, want in ((0, PAIR), (W * H, PAIR), (W * H + 1, FOUR)):
        ctx.set_debug(sva.SVA_DEBUG_DIAG_PAIR_MIN_PIXELS, thr)
        lay = sva.frame_layout(W, H, p, thr)
        assert lay.route == want
        pl = Planes(lay, torch_dev)
        ctx.paths_frame_d(d_C.data_ptr(), d_C.numel(), W, H, p, pl.vol.data_ptr(),
                          lay.volumes_bytes, pl.ck.data_ptr(), lay.ckpt_bytes)
        for u in (0, 10):
            product = ctx.disparity_sgm_conf(L, R, p, u)
            assert ctx.get_debug(sva.SVA_DEBUG_DIAG_ROUTE) == lay.route
            got = run_wta(ctx, pl, d_C, W, H, p, u, True, torch_dev)
            for name, a, b in zip(("disp", "sub", "cost_min", "cost_second"), product, got):
                assert np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else a.dtype),
                                      b.view(np.uint32 if b.dtype == np.float32 else b.dtype)), \
                    (name, thr, u)
            check_outputs(got, e, u)
    # the built-in threshold keeps this small frame on four volumes
    ctx.set_debug(sva.SVA_DEBUG_DIAG_PAIR_MIN_PIXELS, -1)
    assert sva.frame_layout(W, H, p).route == FOUR
    ctx.disparity_sgm_conf(L, R, p, 0)
    assert ctx.get_debug(sva.SVA_DEBUG_DIAG_ROUTE) == FOUR


def test_undersized_buffers_refused(ctx, sva, torch_dev):
    """Each of the three buffers one byte short, or null: SVA_ERR_INVALID_ARG
    from both entries and nothing written."""
    W, H, D = 50, 20, 128
    p = sva.default_params(D=D)
    lay = sva.frame_layout(W, H, p, 0)
    assert lay.route == PAIR
    C = torch.zeros(lay.cost_bytes, dtype=torch.uint8, device=torch_dev)
    pl = Planes(lay, torch_dev)
    disp = torch.full((H, W), 0x1234, dtype=torch.int16, device=torch_dev)
    full = [lay.cost_bytes, lay.volumes_bytes, lay.ckpt_bytes]
    ptrs = [C.data_ptr(), pl.vol.data_ptr(), pl.ck.data_ptr()]
    for i in range(3):
        for null in (False, True):
            sizes, q = list(full), list(ptrs)
            if null:
                q[i] = None
            else:
                sizes[i] -= 1
            with pytest.raises(sva.SvaError) as err:
                ctx.paths_frame_d(q[0], sizes[0], W, H, p, q[1], sizes[1], q[2], sizes[2])
            assert err.value.status == sva.SVA_ERR_INVALID_ARG
            with pytest.raises(sva.SvaError) as err:
                ctx.wta_frame_d(q[0], sizes[0], q[1], sizes[1], q[2], sizes[2], W, H, p, 0,
                                disp.data_ptr())
            assert err.value.status == sva.SVA_ERR_INVALID_ARG
    with pytest.raises(sva.SvaError) as err:
        ctx.wta_frame_d(*[v for pair in zip(ptrs, full) for v in pair], W, H, p, 101, disp.data_ptr())
    assert err.value.status == sva.SVA_ERR_INVALID_ARG
    # a layout of the other route is too small for this one's checkpoint buffer
    four = sva.frame_layout(W, H, p, W * H + 1)
    assert four.route == FOUR and four.ckpt_bytes < lay.ckpt_bytes
    with pytest.raises(sva.SvaError) as err:
        ctx.paths_frame_d(ptrs[0], full[0], W, H, p, ptrs[1], full[1], ptrs[2], four.ckpt_bytes)
    assert err.value.status == sva.SVA_ERR_INVALID_ARG
    pl.fetch(ctx, W, H)
    assert (pl.raw[0] == POISON[0]).all() and (pl.raw[1] == POISON[1]).all()
    assert (host(ctx, disp).view(np.uint16) == 0x1234).all()
