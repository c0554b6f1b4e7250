"""Expected bytes of the tile pipeline's intermediates,
in numpy from the CPU oracle's eight path volumes: the checkpoint rules that
test_tile_stages_gpu.py and test_frame_stages_gpu.py share, and the frame
plan's pair sums, row-checkpoint planes and minima planes.  No fixtures, no GPU
calls."""
import numpy as np

SUB_TOL = 1e-5
MN_SEG = 8             # minima bytes per segment (§4.17)


def path_volumes(oracle, C, P1, P2):
    """L_0 .. L_7 of C [H][W][D] at the caller's D."""
    return [oracle.path(C, r, P1, P2) for r in range(8)]


def volume_sum(vols):
    S = np.zeros(vols[0].shape, np.uint16)
    for v in vols:
        S += v
    return S


def check_checkpoints(hck, vck, vols, seg, nsx, nsy, D=None):
    """hck [2][H][nsx][Dn], vck [2][nsy][W][Dn] against L_0 / L_1 at the
    checkpoint columns and L_2 / L_3 at the checkpoint rows, at d < D."""
    H, W = vols[0].shape[:2]
    d = slice(0, D)
    for s in range(nsx):
        if s * seg + seg < W:          # L_0 at the segment's last column
            assert np.array_equal(hck[0, :, s, d], vols[0][:, s * seg + seg - 1]), ("h0", s)
        if s > 0:                      # L_1 at the segment's first column
            assert np.array_equal(hck[1, :, s, d], vols[1][:, s * seg]), ("h1", s)
    for s in range(nsy):
        if s * seg + seg < H:          # L_2 at the segment's last row
            assert np.array_equal(vck[0, s, :, d], vols[2][s * seg + seg - 1]), ("v0", s)
        if s > 0:                      # L_3 at the segment's first row
            assert np.array_equal(vck[1, s, :, d], vols[3][s * seg]), ("v1", s)


def unwritten_checkpoints(hck, vck):
    """The entries check_checkpoints has no rule for: no kernel writes them."""
    return [hck[0, :, -1], hck[1, :, 0], vck[0, -1], vck[1, 0]]


def check_stages(oracle, C, dmin, res, P1=10, P2=120):
    """sva_paths_tile_d + sva_wta_hv_d: res = (diag, hck, vck, disp, sub, lay)."""
    H, W, D = C.shape
    diag, hck, vck, disp, sub, lay = res
    vols = path_volumes(oracle, C, P1, P2)
    vol_dirs = [4, 5, 6, 7]            # the four diagonal volumes, in direction order
    for slot, r in enumerate(vol_dirs):
        assert np.array_equal(diag[slot], vols[r]), f"direction {r}"
    check_checkpoints(hck, vck, vols, lay.seg, lay.nsx, lay.nsy)
    od, osub = oracle.wta(volume_sum(vols), dmin, True)
    assert np.array_equal(disp, od)
    assert np.max(np.abs(sub - osub)) <= SUB_TOL


def pair_sums(C, vols):
    """The pair route's two volumes (§4.15): E_j = (L_{4+2j} - C) + (L_{5+2j} - C)."""
    c2 = 2 * C.astype(np.int32)
    E = [vols[4].astype(np.int32) + vols[5] - c2, vols[6].astype(np.int32) + vols[7] - c2]
    assert all(e.min() >= 0 and e.max() <= 255 for e in E)
    return [e.astype(np.uint8) for e in E]


def pair_plane_rows(nsy):
    """(down rows, up rows, unwritten rows) of a pair row-checkpoint plane
    [nsy][W][D] (§4.16): the split is at segment q = nsy // 2; the down
    recurrence leaves the last row of segments 0 .. q - 2, the up recurrence
    the first row of segments q + 1 .. nsy - 1, and the states next to the
    split stay in registers."""
    q = nsy // 2
    down = list(range(0, max(q - 1, 0)))
    up = list(range(q + 1, nsy))
    rest = [s for s in range(nsy) if s not in down and s not in up]
    return down, up, rest


def check_pair_planes(pck, vols, seg, D=None):
    """pck [2][nsy][W][Dn]: plane j of the diagonal pair (4 + 2j, 5 + 2j)."""
    d = slice(0, D)
    down, up, _ = pair_plane_rows(pck.shape[1])
    for j in range(2):
        for s in down:
            assert np.array_equal(pck[j, s, :, d], vols[4 + 2 * j][s * seg + seg - 1]), ("down", j, s)
        for s in up:
            assert np.array_equal(pck[j, s, :, d], vols[5 + 2 * j][s * seg]), ("up", j, s)


def entering_minima(vols):
    """ent[r] [H][W], r = 0..3: the minimum the step of direction r into the
    pixel consumed (§4.17): 0 at the line's first pixel, else min_k L_r of the
    line's previous pixel."""
    m = [v.min(axis=2) for v in vols[:4]]
    ent = [np.zeros_like(a) for a in m]
    ent[0][:, 1:] = m[0][:, :-1]
    ent[1][:, :-1] = m[1][:, 1:]
    ent[2][1:] = m[2][:-1]
    ent[3][:-1] = m[3][1:]
    return ent


def minima_planes(vols, nsx, nsy):
    """(hmn [2][H][nsx][8], vmn [2][nsy][W][8], their masks): byte i of a
    segment is its pixel i for directions 0 and 2 and pixel 7 - i for 1 and 3;
    mask = the byte's pixel is inside the image."""
    H, W = vols[0].shape[:2]
    ent = entering_minima(vols)
    hmn = np.zeros((2, H, nsx, MN_SEG), np.uint8)
    vmn = np.zeros((2, nsy, W, MN_SEG), np.uint8)
    hmask, vmask = np.zeros(hmn.shape, bool), np.zeros(vmn.shape, bool)
    for r in range(2):
        for s in range(nsx):
            for i in range(MN_SEG):
                x = s * MN_SEG + (i if r == 0 else MN_SEG - 1 - i)
                if x < W:
                    hmn[r, :, s, i] = ent[r][:, x]
                    hmask[r, :, s, i] = True
        for s in range(nsy):
            for i in range(MN_SEG):
                y = s * MN_SEG + (i if r == 0 else MN_SEG - 1 - i)
                if y < H:
                    vmn[r, s, :, i] = ent[2 + r][y]
                    vmask[r, s, :, i] = True
    return hmn, vmn, hmask, vmask


def pair_line_wraps_inside_segment(W, H, seg=8):
    """Some pair line of a W x H frame crosses the image edge between two rows
    of one segment (its column wraps there and the recurrences restart)."""
    for line in range(W):
        for y in range(H - 1):
            if y % seg != seg - 1 and (line + y) % W == W - 1:
                return True
    return False
