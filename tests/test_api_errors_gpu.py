"""Rejected calls of the C-ABI (include/sva.h): one row per distinct argument
check of the entry points that come as a host-buffer / device-buffer (`_d`)
pair, of the batch and confidence entries, and of the stage entries that share
check_sgm / check_tile_buffers.

Each row names the one bad argument, the status and the exact sva_last_error
text; every other argument is valid (the `_d` form gets real device buffers of
the right size, so a check that went missing fails the test instead of handing
a bad pointer to a kernel).  Pairs are asserted in both forms: the host form
and its `_d` twin refuse the same call with the same status and text.  Every
row is refused before any allocation or launch, so the test runs in
milliseconds."""
import ctypes as ct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INV, UNS = 1, 2          # SVA_ERR_INVALID_ARG, SVA_ERR_UNSUPPORTED
W0, H0 = 24, 16

M_IMG_NULL = "null image pointer"
M_SIZE = "image size must be positive"
M_PITCH = "pitch smaller than width"
M_PARAMS = "null params"
M_D_POS = "D must be positive"
M_D_MAX = "GPU path built for D in 1..256"
M_D_NATIVE = "stage entry points take D in {64,128,192,256} (whole frames: any D <= 256)"
M_STEP = "(dir, dir_y) must be a nonzero step, |comp| <= 255"
M_DMIN = "dmin must be >= 0"
M_DMIN_D = "dmin + D must fit the u16 disparity map"
M_PEN = "penalties must satisfy 0 <= P1, P2 <= 193"
M_LRDIFF = "lr_max_diff must be >= 0"
M_H = "H must be <= 65535"
M_VOL = "W*H*D must be < 2^32 (32-bit volume offsets)"
M_DISP = "null disparity output"
M_UNIQ = "uniqueness must be 0..100 (percent, 0 = off)"
M_BATCH = "bad batch argument"
M_SHARE = "a batch's pairs must share D, dmin, P1, P2 and subpixel"
M_SHARE_INV = "a confidence batch's pairs must share invalid"
M_BATCH_LR = "the batch route has no L/R check"
M_BAD = "bad argument"
M_SPLIT = ("census+cost kernel: D in {64,128,192,256}, 1-D steps or 2-D steps whose "
           "primitive form has |dir_y| = 1 and |dir| <= 3")
M_STAGE_NULL = "null stage buffer"
M_CAM = "null camera"
M_PLANE = "null plane"
M_H_GRID = "H must be <= 65535 (gridDim.y)"
M_DIMS = "matrix dimensions must be positive (< 2^31 elements)"
M_MATRIX = "null matrix"
M_NMAPS = "n_maps must be 1..32"


class Env:
    """Buffers of one form: numpy arrays (host) or torch tensors (device)."""

    def __init__(self, sva, dev, form):
        self.sva, self.dev, self.form = sva, dev, form

    def buf(self, nbytes):
        if self.form == "host":
            return np.zeros(nbytes, np.uint8)
        return torch.zeros(nbytes, dtype=torch.uint8, device=self.dev)

    def cam(self):
        return self.sva.Camera.make(0.05, (0.0, 0.0, 0.0), 2e-5)


# ---- valid arguments of each entry point, in the order of its signature ----
def b_sgm(E, W, H):
    n = W * H
    return dict(left=E.buf(n), right=E.buf(n), W=W, H=H, pitch=W,
                p=E.sva.default_params(D=64, subpixel=1), disp=E.buf(2 * n), sub=E.buf(4 * n))


def b_sgm_conf(E, W, H):
    a = b_sgm(E, W, H)
    disp, sub = a.pop("disp"), a.pop("sub")
    a.update(uniqueness=10, disp=disp, sub=sub, cost_min=E.buf(2 * W * H),
             cost_second=E.buf(2 * W * H))
    return a


def b_batch(E, W, H, conf=False):
    n = W * H
    keep = [E.buf(n) for _ in range(4)]
    jobs = (E.sva.PairD * 2)()
    for i in range(2):
        jobs[i] = E.sva.PairD(E.sva._ptr(keep[2 * i]), E.sva._ptr(keep[2 * i + 1]),
                              E.sva.default_params(D=64, subpixel=1))
    a = dict(jobs=jobs, n=2, W=W, H=H, pitch=W)
    if conf:
        a["uniqueness"] = 10
    a.update(maps=E.buf(4 * n), sub=E.buf(8 * n))
    if conf:
        a.update(cost_min=E.buf(4 * n), cost_second=E.buf(4 * n))
    a["_keep"] = keep
    return a


def b_batch_conf(E, W, H):
    return b_batch(E, W, H, conf=True)


def b_cost(E, W, H):
    n = W * H
    return dict(cl=E.buf(8 * n), cr=E.buf(8 * n), W=W, H=H, p=E.sva.default_params(D=64),
                C=E.buf(64 * n))


def b_census_cost(E, W, H):
    n = W * H
    return dict(left=E.buf(n), right=E.buf(n), W=W, H=H, pitch=W, p=E.sva.default_params(D=64),
                C=E.buf(64 * n))


def b_paths(E, W, H):
    n = W * H
    return dict(C=E.buf(64 * n), W=W, H=H, p=E.sva.default_params(D=64), L8=E.buf(8 * 64 * n))


def b_aggregate(E, W, H):
    n = W * H
    return dict(C=E.buf(64 * n), W=W, H=H, p=E.sva.default_params(D=64), S=E.buf(2 * 64 * n))


def b_wta(E, W, H):
    n = W * H
    return dict(S=E.buf(2 * 64 * n), W=W, H=H, p=E.sva.default_params(D=64, subpixel=1),
                disp=E.buf(2 * n), sub=E.buf(4 * n))


def b_wta_conf(E, W, H):
    n = W * H
    return dict(S=E.buf(2 * 64 * n), W=W, H=H, p=E.sva.default_params(D=64, subpixel=1),
                uniqueness=10, disp=E.buf(2 * n), sub=E.buf(4 * n), cost_min=E.buf(2 * n),
                cost_second=E.buf(2 * n))


def b_paths_tile(E, W, H):
    l = E.sva.tile_layout(W, H, 64)
    return dict(C=E.buf(l.cost_bytes), C_bytes=l.cost_bytes, W=W, H=H,
                p=E.sva.default_params(D=64), diag=E.buf(l.diag_bytes), diag_bytes=l.diag_bytes,
                hck=E.buf(l.hckpt_bytes), hck_bytes=l.hckpt_bytes, vck=E.buf(l.vckpt_bytes),
                vck_bytes=l.vckpt_bytes)


def b_wta_hv(E, W, H):
    l = E.sva.tile_layout(W, H, 64)
    return dict(C=E.buf(l.cost_bytes), C_bytes=l.cost_bytes, diag=E.buf(l.diag_bytes),
                diag_bytes=l.diag_bytes, hck=E.buf(l.hckpt_bytes), hck_bytes=l.hckpt_bytes,
                vck=E.buf(l.vckpt_bytes), vck_bytes=l.vckpt_bytes, W=W, H=H,
                p=E.sva.default_params(D=64, subpixel=1), disp=E.buf(2 * W * H),
                sub=E.buf(4 * W * H))


def b_ref(E, W, H):
    n = W * H
    return dict(ref=E.buf(n), other=E.buf(n), W=W, H=H, pitch=W, mask=None, cref=E.cam(),
                coth=E.cam(), k=2, t_near=0.5, t_far=1.0, d8=E.buf(n), d16=E.buf(2 * n),
                valid=E.buf(n))


def b_ref_endpoints(E, W, H):
    n = W * H
    return dict(W=W, H=H, cref=E.cam(), coth=E.cam(), k=2, t_near=0.5, t_far=1.0,
                ends=E.buf(16 * n), valid=E.buf(n))


def b_to_depth(E, W, H):
    return dict(disp=E.buf(W * H), n=W * H, cam_distance=0.05, f=0.05, pixel_size=2e-5,
                depth=E.buf(8 * W * H))


def b_fuse(E, W, H):
    n = W * H
    return dict(disps=E.buf(2 * n * 33), n_maps=2, W=W, H=H, baselines=(ct.c_double * 33)(*[0.05] * 33),
                f=0.05, pixel_size=2e-5, invalid=0xFFFF, depth=E.buf(8 * n), n_valid=E.buf(n))


def b_fuse_conf(E, W, H):
    n = W * H
    return dict(disps=E.buf(2 * n * 33), cost_min=E.buf(2 * n * 33), cost_second=E.buf(2 * n * 33),
                n_maps=2, W=W, H=H, baselines=(ct.c_double * 33)(*[0.05] * 33), f=0.05,
                pixel_size=2e-5, invalid=0xFFFF, mode=0, depth=E.buf(8 * n), n_valid=E.buf(n),
                winner=E.buf(n))


def b_shift(E, W, H):
    n = W * H
    return dict(in_cam=E.cam(), out_cam=E.cam(), disparity=E.buf(n), image=E.buf(n), W=W, H=H,
                pitch=W, shifted=E.buf(n))


def b_improve(E, W, H):
    n = W * H
    img = E.buf(n)
    return dict(disparity=E.buf(n), center=E.buf(n), images=(ct.c_void_p * 1)(E.sva._ptr(img)),
                cam_pairs=(E.sva.Camera * 2)(E.cam(), E.cam()), n_pairs=1, W=W, H=H, pitch=W,
                mask=None, window_size=3, strict=0, out=E.buf(n), _keep=img)


def b_shift2(E, W, H):
    n = W * H
    return dict(in_cam=E.cam(), out_cam=E.cam(), depth=E.buf(8 * n), W=W, H=H,
                shifted=E.buf(8 * n))


def b_points_to_depth(E, W, H):
    return dict(points=E.buf(24 * 5), n_points=5, cam=E.cam(), W=W, H=H, depth=E.buf(8 * W * H))


def b_depth_to_points(E, W, H):
    n = W * H
    return dict(depth=E.buf(8 * n), W=W, H=H, cam=E.cam(), points=E.buf(24 * n),
                n_points=ct.c_int64(0))


def b_resize_half(E, W, H):
    dw, dh = E.sva.resize_half_size(W, H)
    return dict(src=E.buf(W * H), W=W, H=H, pitch=W, dst=E.buf(dw * dh), dst_pitch=dw)


def b_resize_linear(E, W, H):
    return dict(src=E.buf(8 * W * H), sw=W, sh=H, dst=E.buf(8 * 10 * 7), dw=10, dh=7)


def b_ref_error(E, W, H):
    return dict(depth=E.buf(8 * W * H), w=W, h=H, ref=E.buf(8 * 10 * 7), rw=10, rh=7, scale=50.0,
                error=E.buf(8 * 10 * 7))


def b_masked_mean(E, W, H):
    return dict(image=E.buf(8 * W * H), mask=None, w=W, h=H, mean=ct.c_double(0))


# entry -> (symbol of the host form or None, symbol of the _d form, builder)
ENTRIES = {
    "sgm": ("sva_disparity_sgm", "sva_disparity_sgm_d", b_sgm),
    "sgm_conf": ("sva_disparity_sgm_conf", "sva_disparity_sgm_conf_d", b_sgm_conf),
    "batch": (None, "sva_disparity_sgm_batch_d", b_batch),
    "batch_conf": (None, "sva_disparity_sgm_batch_conf_d", b_batch_conf),
    "cost": (None, "sva_cost_d", b_cost),
    "census_cost": (None, "sva_census_cost_d", b_census_cost),
    "paths": (None, "sva_paths_d", b_paths),
    "aggregate": (None, "sva_aggregate_d", b_aggregate),
    "wta": (None, "sva_wta_d", b_wta),
    "wta_conf": (None, "sva_wta_conf_d", b_wta_conf),
    "paths_tile": (None, "sva_paths_tile_d", b_paths_tile),
    "wta_hv": (None, "sva_wta_hv_d", b_wta_hv),
    "ref": ("sva_disparity_ref", "sva_disparity_ref_d", b_ref),
    "ref_endpoints": (None, "sva_ref_endpoints_d", b_ref_endpoints),
    "to_depth": ("sva_disparity_to_depth", "sva_disparity_to_depth_d", b_to_depth),
    "fuse": ("sva_fuse_depth", "sva_fuse_depth_d", b_fuse),
    "fuse_conf": ("sva_fuse_depth_conf", "sva_fuse_depth_conf_d", b_fuse_conf),
    "shift": ("sva_shift_perspective", "sva_shift_perspective_d", b_shift),
    "improve": ("sva_improve_with_disparity", "sva_improve_with_disparity_d", b_improve),
    "shift2": ("sva_shift_perspective2", "sva_shift_perspective2_d", b_shift2),
    "points_to_depth": ("sva_points_to_depth", "sva_points_to_depth_d", b_points_to_depth),
    "depth_to_points": ("sva_depth_to_points", "sva_depth_to_points_d", b_depth_to_points),
    "resize_half": ("sva_resize_half", "sva_resize_half_d", b_resize_half),
    "resize_linear": ("sva_resize_linear_f64", "sva_resize_linear_f64_d", b_resize_linear),
    "ref_error": ("sva_ref_error", "sva_ref_error_d", b_ref_error),
    "masked_mean": ("sva_masked_mean", "sva_masked_mean_d", b_masked_mean),
}

# (entry, bad arguments, status, sva_last_error).  A dotted key reaches into a
# struct or an array ("p.D", "jobs.1.params.D"); "shape": (W, H) sizes the
# buffers for a shape other than W0 x H0.  Rows with two bad arguments pin the
# order of the checks.
ROWS = [
    # sva_disparity_sgm[_d]: check_image on both images, every check_sgm clause
    ("sgm", {"left": None}, INV, M_IMG_NULL),
    ("sgm", {"right": None}, INV, M_IMG_NULL),
    ("sgm", {"W": 0}, INV, M_SIZE),
    ("sgm", {"H": -1}, INV, M_SIZE),
    ("sgm", {"pitch": W0 - 1}, INV, M_PITCH),
    ("sgm", {"p": None}, INV, M_PARAMS),
    ("sgm", {"p.D": 0}, INV, M_D_POS),
    ("sgm", {"p.D": 257}, UNS, M_D_MAX),
    ("sgm", {"p.dir": 0}, INV, M_STEP),
    ("sgm", {"p.dir": 256}, INV, M_STEP),
    ("sgm", {"p.dir_y": -256}, INV, M_STEP),
    ("sgm", {"p.dmin": -1}, INV, M_DMIN),
    ("sgm", {"p.dmin": 65472}, INV, M_DMIN_D),
    ("sgm", {"p.P1": -1}, INV, M_PEN),
    ("sgm", {"p.P2": 194}, INV, M_PEN),
    ("sgm", {"p.lr_check": 1, "p.lr_max_diff": -1}, INV, M_LRDIFF),
    ("sgm", {"shape": (1, 65536)}, UNS, M_H),
    ("sgm", {"shape": (4096, 4096), "p.D": 256}, UNS, M_VOL),
    ("sgm", {"disp": None}, INV, M_DISP),
    ("sgm", {"left": None, "p": None}, INV, M_IMG_NULL),
    ("sgm", {"p.D": 0, "disp": None}, INV, M_D_POS),
    # the confidence form: the same checks, then uniqueness, then the output
    ("sgm_conf", {"left": None}, INV, M_IMG_NULL),
    ("sgm_conf", {"H": 0}, INV, M_SIZE),
    ("sgm_conf", {"pitch": W0 - 1}, INV, M_PITCH),
    ("sgm_conf", {"p": None}, INV, M_PARAMS),
    ("sgm_conf", {"p.D": 257}, UNS, M_D_MAX),
    ("sgm_conf", {"p.P2": 194}, INV, M_PEN),
    ("sgm_conf", {"uniqueness": -1}, INV, M_UNIQ),
    ("sgm_conf", {"uniqueness": 101}, INV, M_UNIQ),
    ("sgm_conf", {"disp": None}, INV, M_DISP),
    ("sgm_conf", {"uniqueness": 101, "disp": None}, INV, M_UNIQ),
    ("sgm_conf", {"p.dmin": -1, "uniqueness": 101}, INV, M_DMIN),
    # the batch entries
    ("batch", {"jobs": None}, INV, M_BATCH),
    ("batch", {"n": 0}, INV, M_BATCH),
    ("batch", {"maps": None}, INV, M_BATCH),
    ("batch", {"jobs.1.left": None}, INV, M_IMG_NULL),
    ("batch", {"jobs.0.right": None}, INV, M_IMG_NULL),
    ("batch", {"W": 0}, INV, M_SIZE),
    ("batch", {"pitch": W0 - 1}, INV, M_PITCH),
    ("batch", {"jobs.1.params.dir": 0}, INV, M_STEP),
    ("batch", {"jobs.0.params.D": 257, "jobs.1.params.D": 257}, UNS, M_D_MAX),
    ("batch", {"jobs.1.params.D": 128}, INV, M_SHARE),
    ("batch", {"jobs.1.params.dmin": 3}, INV, M_SHARE),
    ("batch", {"jobs.1.params.P1": 11}, INV, M_SHARE),
    ("batch", {"jobs.1.params.P2": 100}, INV, M_SHARE),
    ("batch", {"jobs.1.params.subpixel": 0}, INV, M_SHARE),
    ("batch", {"jobs.1.params.lr_check": 1}, UNS, M_BATCH_LR),
    ("batch", {"jobs.0.params.lr_check": 1, "jobs.1.params.D": 128}, UNS, M_BATCH_LR),
    ("batch_conf", {"jobs": None}, INV, M_BATCH),
    ("batch_conf", {"n": -1}, INV, M_BATCH),
    ("batch_conf", {"maps": None}, INV, M_BATCH),
    ("batch_conf", {"uniqueness": -1}, INV, M_UNIQ),
    ("batch_conf", {"uniqueness": 101}, INV, M_UNIQ),
    ("batch_conf", {"uniqueness": 101, "jobs.0.left": None}, INV, M_UNIQ),
    ("batch_conf", {"jobs.1.right": None}, INV, M_IMG_NULL),
    ("batch_conf", {"jobs.1.params.D": 0}, INV, M_D_POS),
    ("batch_conf", {"jobs.1.params.D": 128}, INV, M_SHARE),
    ("batch_conf", {"jobs.1.params.invalid": 0xFFFE}, INV, M_SHARE_INV),
    ("batch_conf", {"jobs.1.params.invalid": 0xFFFE, "jobs.1.params.lr_check": 1}, INV, M_SHARE_INV),
    ("batch_conf", {"jobs.1.params.lr_check": 1}, UNS, M_BATCH_LR),
    # stage entries on check_sgm(native)
    ("cost", {"p": None}, INV, M_PARAMS),
    ("cost", {"p.D": 100}, UNS, M_D_NATIVE),
    ("cost", {"cl": None}, INV, M_BAD),
    ("cost", {"C": None}, INV, M_BAD),
    ("cost", {"W": 0}, INV, M_BAD),
    ("census_cost", {"p": None}, INV, M_PARAMS),
    ("census_cost", {"p.D": 100}, UNS, M_D_NATIVE),
    ("census_cost", {"p": None, "left": None}, INV, M_PARAMS),
    ("census_cost", {"left": None}, INV, M_IMG_NULL),
    ("census_cost", {"right": None}, INV, M_IMG_NULL),
    ("census_cost", {"pitch": W0 - 1}, INV, M_PITCH),
    ("census_cost", {"C": None}, INV, "null cost output"),
    ("census_cost", {"p.dir": 1, "p.dir_y": 3}, UNS, M_SPLIT),
    ("census_cost", {"p.dir": 4, "p.dir_y": 1}, UNS, M_SPLIT),
    ("census_cost", {"p.dir": 1, "p.dir_y": 3, "C": None}, INV, "null cost output"),
    ("paths", {"p.D": 100}, UNS, M_D_NATIVE),
    ("paths", {"p.P1": 194}, INV, M_PEN),
    ("paths", {"C": None}, INV, M_BAD),
    ("paths", {"L8": None}, INV, M_BAD),
    ("aggregate", {"p.D": 65}, UNS, M_D_NATIVE),
    ("aggregate", {"S": None}, INV, M_BAD),
    ("aggregate", {"H": 0}, INV, M_BAD),
    ("wta", {"p.dmin": -1}, INV, M_DMIN),
    ("wta", {"S": None}, INV, M_BAD),
    ("wta", {"disp": None}, INV, M_BAD),
    ("wta_conf", {"p.D": 100}, UNS, M_D_NATIVE),
    ("wta_conf", {"uniqueness": -1}, INV, M_UNIQ),
    ("wta_conf", {"uniqueness": 101, "S": None}, INV, M_UNIQ),
    ("wta_conf", {"S": None}, INV, M_BAD),
    ("wta_conf", {"disp": None}, INV, M_BAD),
    # stage entries on check_tile_buffers
    ("paths_tile", {"p": None}, INV, M_PARAMS),
    ("paths_tile", {"p.D": 100}, UNS, M_D_NATIVE),
    ("paths_tile", {"C": None}, INV, M_STAGE_NULL),
    ("paths_tile", {"diag": None}, INV, M_STAGE_NULL),
    ("paths_tile", {"hck": None}, INV, M_STAGE_NULL),
    ("paths_tile", {"vck": None}, INV, M_STAGE_NULL),
    ("paths_tile", {"C_bytes": W0 * H0 * 64 - 1}, INV, "cost buffer smaller than [H][W][D]"),
    ("paths_tile", {"diag_bytes": 4 * W0 * H0 * 64 - 1}, INV,
     "diagonal volume buffer smaller than [4][H][W][D]"),
    ("paths_tile", {"hck_bytes": 1}, INV,
     "horizontal checkpoint buffer smaller than [2][H][nsx][D]"),
    ("paths_tile", {"vck_bytes": 1}, INV, "row checkpoint buffer smaller than [2][nsy][W][D]"),
    ("wta_hv", {"p.dir": 0}, INV, M_STEP),
    ("wta_hv", {"vck": None}, INV, M_STAGE_NULL),
    ("wta_hv", {"C_bytes": 0}, INV, "cost buffer smaller than [H][W][D]"),
    ("wta_hv", {"diag_bytes": 4 * W0 * H0 * 64 - 1}, INV,
     "diagonal volume buffer smaller than [4][H][W][D]"),
    ("wta_hv", {"disp": None}, INV, M_DISP),
    ("wta_hv", {"vck_bytes": 1, "disp": None}, INV,
     "row checkpoint buffer smaller than [2][nsy][W][D]"),
    # Mode R
    ("ref", {"ref": None}, INV, M_IMG_NULL),
    ("ref", {"other": None}, INV, M_IMG_NULL),
    ("ref", {"W": 0}, INV, M_SIZE),
    ("ref", {"pitch": W0 - 1}, INV, M_PITCH),
    ("ref", {"cref": None}, INV, M_CAM),
    ("ref", {"coth": None}, INV, M_CAM),
    ("ref", {"k": 0}, INV, "kernel half-size k must be >= 1"),
    ("ref", {"k": W0 // 2}, INV, "image smaller than window"),
    ("ref", {"k": H0 // 2}, INV, "image smaller than window"),
    ("ref", {"t_near": 0.0}, INV, "ray parameters must be positive"),
    ("ref", {"t_far": -1.0}, INV, "ray parameters must be positive"),
    ("ref", {"shape": (32768, 8)}, UNS, "Mode R supports W, H <= 32767"),
    ("ref", {"d8": None}, INV, M_DISP),
    ("ref", {"k": 0, "d8": None}, INV, "kernel half-size k must be >= 1"),
    ("ref_endpoints", {"cref": None}, INV, M_CAM),
    ("ref_endpoints", {"k": 0}, INV, "kernel half-size k must be >= 1"),
    ("ref_endpoints", {"t_near": -0.5}, INV, "ray parameters must be positive"),
    ("ref_endpoints", {"ends": None}, INV, "null output"),
    ("ref_endpoints", {"valid": None}, INV, "null output"),
    # disparity -> depth and the fusions
    ("to_depth", {"disp": None}, INV, M_BAD),
    ("to_depth", {"depth": None}, INV, M_BAD),
    ("to_depth", {"n": -1}, INV, M_BAD),
    ("fuse", {"disps": None}, INV, "null pointer"),
    ("fuse", {"baselines": None}, INV, "null pointer"),
    ("fuse", {"depth": None}, INV, "null pointer"),
    ("fuse", {"n_maps": 0}, UNS, M_NMAPS),
    ("fuse", {"n_maps": 33}, UNS, M_NMAPS),
    ("fuse", {"W": 0}, INV, M_SIZE),
    ("fuse", {"n_maps": 33, "H": 0}, UNS, M_NMAPS),
    ("fuse_conf", {"disps": None}, INV, "null pointer"),
    ("fuse_conf", {"cost_min": None}, INV, "null pointer"),
    ("fuse_conf", {"baselines": None}, INV, "null pointer"),
    ("fuse_conf", {"depth": None}, INV, "null pointer"),
    ("fuse_conf", {"mode": 2}, INV, "mode must be SVA_FUSE_MIN_COST or SVA_FUSE_MAX_MARGIN"),
    ("fuse_conf", {"mode": -1}, INV, "mode must be SVA_FUSE_MIN_COST or SVA_FUSE_MAX_MARGIN"),
    ("fuse_conf", {"mode": 1, "cost_second": None}, INV,
     "SVA_FUSE_MAX_MARGIN needs the cost_second planes"),
    ("fuse_conf", {"n_maps": 0}, INV, M_NMAPS),
    ("fuse_conf", {"n_maps": 33}, INV, M_NMAPS),
    ("fuse_conf", {"H": 0}, INV, M_SIZE),
    ("fuse_conf", {"mode": 2, "n_maps": 0}, INV,
     "mode must be SVA_FUSE_MIN_COST or SVA_FUSE_MAX_MARGIN"),
    # refinement / 3-D
    ("shift", {"W": 0}, INV, M_SIZE),
    ("shift", {"pitch": W0 - 1}, INV, M_PITCH),
    ("shift", {"shape": (1, 65536)}, UNS, M_H_GRID),
    ("shift", {"in_cam": None}, INV, M_CAM),
    ("shift", {"out_cam": None}, INV, M_CAM),
    ("shift", {"disparity": None}, INV, M_PLANE),
    ("shift", {"image": None}, INV, M_PLANE),
    ("shift", {"shifted": None}, INV, M_PLANE),
    ("shift", {"in_cam": None, "shifted": None}, INV, M_CAM),
    ("improve", {"H": 0}, INV, M_SIZE),
    ("improve", {"pitch": W0 - 1}, INV, M_PITCH),
    ("improve", {"window_size": 0}, UNS, "window_size must be >= 1"),
    ("improve", {"n_pairs": -1}, INV, "bad pair list"),
    ("improve", {"images": None}, INV, "bad pair list"),
    ("improve", {"cam_pairs": None}, INV, "bad pair list"),
    ("improve", {"disparity": None}, INV, M_PLANE),
    ("improve", {"center": None}, INV, M_PLANE),
    ("improve", {"out": None}, INV, M_PLANE),
    ("improve", {"images.0": None}, INV, "null pair image"),
    ("improve", {"window_size": 0, "out": None}, UNS, "window_size must be >= 1"),
    ("improve", {"images.0": None, "out": None}, INV, M_PLANE),
    ("shift2", {"W": -3}, INV, M_SIZE),
    ("shift2", {"in_cam": None}, INV, M_CAM),
    ("shift2", {"out_cam": None}, INV, M_CAM),
    ("shift2", {"depth": None}, INV, M_PLANE),
    ("shift2", {"shifted": None}, INV, M_PLANE),
    ("points_to_depth", {"H": 0}, INV, M_SIZE),
    ("points_to_depth", {"cam": None}, INV, M_CAM),
    ("points_to_depth", {"n_points": -1}, INV, "bad point list"),
    ("points_to_depth", {"points": None}, INV, "bad point list"),
    ("points_to_depth", {"depth": None}, INV, "bad point list"),
    ("depth_to_points", {"W": 0}, INV, M_SIZE),
    ("depth_to_points", {"cam": None}, INV, M_CAM),
    ("depth_to_points", {"depth": None}, INV, "null argument"),
    ("depth_to_points", {"points": None}, INV, "null argument"),
    ("depth_to_points", {"n_points": None}, INV, "null argument"),
    # ingestion and evaluation
    ("resize_half", {"W": 0}, INV, M_SIZE),
    ("resize_half", {"pitch": W0 - 1}, INV, M_PITCH),
    ("resize_half", {"src": None}, INV, "bad resize argument"),
    ("resize_half", {"dst": None}, INV, "bad resize argument"),
    ("resize_half", {"dst_pitch": W0 // 2 - 1}, INV, "bad resize argument"),
    ("resize_linear", {"sw": 0}, INV, M_DIMS),
    ("resize_linear", {"dh": 0}, INV, M_DIMS),
    ("resize_linear", {"src": None}, INV, M_MATRIX),
    ("resize_linear", {"dst": None}, INV, M_MATRIX),
    ("ref_error", {"w": 0}, INV, M_DIMS),
    ("ref_error", {"rh": -1}, INV, M_DIMS),
    ("ref_error", {"depth": None}, INV, M_MATRIX),
    ("ref_error", {"ref": None}, INV, M_MATRIX),
    ("ref_error", {"error": None}, INV, M_MATRIX),
    ("masked_mean", {"w": 0}, INV, M_DIMS),
    ("masked_mean", {"image": None}, INV, "null argument"),
    ("masked_mean", {"mean": None}, INV, "null argument"),
]


def put(args, key, value):
    """args[key] = value, a dotted key walking into structs and arrays."""
    parts = key.split(".")
    if len(parts) == 1:
        args[key] = value
        return
    obj = args[parts[0]]
    for part in parts[1:-1]:
        obj = obj[int(part)] if part.isdigit() else getattr(obj, part)
    if parts[-1].isdigit():
        obj[int(parts[-1])] = value
    else:
        setattr(obj, parts[-1], value)


def to_c(sva, v):
    if isinstance(v, (np.ndarray, torch.Tensor)):
        return sva._ptr(v)
    if isinstance(v, (sva.SgmParams, sva.Camera, ct.c_int64, ct.c_double)):
        return ct.byref(v)
    return v


def case_id(row):
    return row[0] + ":" + ",".join(f"{k}={v}" for k, v in row[1].items())


CASES = [(row, form) for row in ROWS for form in ("host", "d")
         if form == "d" or ENTRIES[row[0]][0] is not None]


@pytest.mark.parametrize("row,form", CASES, ids=[f"{case_id(r)}-{f}" for r, f in CASES])
def test_rejected_call(ctx, sva, torch_dev, row, form):
    entry, bad, status, message = row
    host_sym, dev_sym, build = ENTRIES[entry]
    bad = dict(bad)
    W, H = bad.pop("shape", (W0, H0))
    args = build(Env(sva, torch_dev, form), W, H)
    for key, value in bad.items():
        put(args, key, value)
    call = [to_c(sva, v) for k, v in args.items() if not k.startswith("_")]
    got = getattr(sva.lib, host_sym if form == "host" else dev_sym)(ctx.h, *call)
    text = sva.lib.sva_last_error(ctx.h).decode()
    assert (got, text) == (status, message)


def test_table_covers_every_entry():
    assert {r[0] for r in ROWS} == set(ENTRIES)
