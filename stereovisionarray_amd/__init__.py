"""stereovisionarray_amd -- MI355X-native stereo disparity engine.

The product is the C-ABI shared library ``libsva.so`` (hand-written HIP
kernels for gfx950 + a C++ host layer, declared in ``include/sva.h``).  This
module is a thin ctypes binding used by the tests and ``bench.py``; it adds no
compute of its own and has no CPU fallback: if ``libsva.so`` is missing, import
fails loudly, and if no GPU is present every compute call raises.

Host-pointer calls take numpy arrays; ``*_d`` calls take device pointers
(ints), e.g. ``torch_tensor.data_ptr()``.
"""
from __future__ import annotations

import ctypes as ct
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SVA_LIB_PATH: load an alternative build of the same library (kernel-variant
# experiments under tools/); the default is the in-tree libsva.so.
LIB_PATH = os.environ.get("SVA_LIB_PATH") or os.path.join(_HERE, "libsva.so")

SVA_OK = 0
SVA_ERR_INVALID_ARG = 1
SVA_ERR_UNSUPPORTED = 2
SVA_ERR_DEVICE = 3
SVA_ERR_OUT_OF_MEMORY = 4
SVA_ERR_NO_DEVICE = 5
SVA_PATH_KERNEL_COST_VOLUME = 0
SVA_PATH_KERNEL_FUSED = 1
SVA_PATH_KERNEL_AUTO = 2
SVA_TIMING_OFF = 0
SVA_TIMING_ALL = 1
SVA_TIMING_PATHS = 2
SVA_TIMING_AGG = 3
SVA_DEBUG_PLANE_SPLIT = 1
SVA_DEBUG_FAIL_COST_AT = 2
SVA_DEBUG_SIDE_IDLE = 3
SVA_DEBUG_PLACEMENT_TRIALS = 4
SVA_DEBUG_PLACEMENT_NS = 5
SVA_DEBUG_PLACEMENT_WORST_NS = 6
SVA_DEBUG_DIAG_ROUTE = 7
SVA_DEBUG_DIAG_PAIR_MIN_PIXELS = 8
SVA_DEBUG_REFINE_ROUTE = 9
SVA_DEBUG_REFINE_LAST_ROUTE = 10
SVA_DEBUG_CROSS_ORDER = 11
SVA_DEBUG_FILL_SEGMENT = 12
# The ABI this binding is written against (include/sva.h SVA_ABI_VERSION).
ABI_VERSION = 6

# Symbols declared in include/sva.h (checked by tests/test_abi.py).
EXPORTED = [
    "sva_sgm_params_default", "sva_abi_version", "sva_device_count", "sva_create",
    "sva_destroy", "sva_set_stream", "sva_synchronize", "sva_last_error",
    "sva_status_string", "sva_reserve", "sva_set_path_kernel", "sva_set_timing", "sva_reset_timing",
    "sva_kernel_time", "sva_disparity_sgm", "sva_disparity_sgm_d", "sva_census_d",
    "sva_cost_d", "sva_census_cost_d", "sva_paths_d", "sva_aggregate_d", "sva_wta_d", "sva_disparity_ref",
    "sva_disparity_ref_d", "sva_ref_endpoints_d", "sva_disparity_to_depth_d",
    "sva_disparity_to_depth", "sva_fuse_depth_d", "sva_fuse_depth",
    "sva_shift_perspective_d", "sva_shift_perspective", "sva_improve_with_disparity_d",
    "sva_improve_with_disparity", "sva_shift_perspective2_d", "sva_shift_perspective2",
    "sva_points_to_depth_d", "sva_points_to_depth", "sva_depth_to_points_d",
    "sva_depth_to_points", "sva_resize_half_size", "sva_resize_half_d", "sva_resize_half",
    "sva_batch_sgm", "sva_resize_linear_f64_d", "sva_resize_linear_f64", "sva_ref_error_d",
    "sva_ref_error", "sva_masked_mean_d", "sva_masked_mean", "sva_tile_layout_of",
    "sva_tile_check", "sva_paths_tile_d", "sva_wta_hv_d", "sva_multi_create", "sva_multi_destroy",
    "sva_multi_synchronize", "sva_multi_last_error", "sva_multi_plan", "sva_multi_context",
    "sva_batch_sgm_d", "sva_array_depth", "sva_disparity_sgm_batch_d", "sva_set_debug",
    "sva_get_debug", "sva_disparity_sgm_conf", "sva_disparity_sgm_conf_d", "sva_wta_conf_d",
    "sva_fuse_depth_conf", "sva_fuse_depth_conf_d", "sva_disparity_sgm_batch_conf_d",
    "sva_batch_sgm_conf_d", "sva_array_depth_conf", "sva_cost_fuse_d", "sva_disparity_sgm_multi",
    "sva_disparity_sgm_multi_d", "sva_array_depth_mb", "sva_cost_mixed_d",
    "sva_cost_fuse_mixed_d", "sva_disparity_sgm_mixed", "sva_disparity_sgm_mixed_d",
    "sva_array_depth_mixed", "sva_frame_layout_of", "sva_paths_frame_d", "sva_wta_frame_d",
    "sva_fuse_depth_sub", "sva_fuse_depth_sub_d", "sva_fuse_depth_conf_sub",
    "sva_fuse_depth_conf_sub_d", "sva_array_depth_sub", "sva_cross_check", "sva_cross_check_d",
    "sva_array_depth_checked", "sva_filter_speckles", "sva_filter_speckles_d",
    "sva_array_depth_filtered", "sva_fill_holes", "sva_fill_holes_d", "sva_array_depth_filled",
    "sva_weighted_median", "sva_weighted_median_d", "sva_array_depth_smoothed",
    "sva_rectify", "sva_rectify_d", "sva_rectify_view_of", "sva_mask_maps", "sva_mask_maps_d",
    "sva_array_depth_rectified",
]
SVA_RECTIFY_MAX_SIZE = 32767
SVA_WMED_MAX_RADIUS = 15
SVA_FILL_MIN = 0
SVA_FILL_SECOND = 1
SVA_FILL_MEDIAN = 2
SVA_FILL_MAX_DIST = 255
SVA_FUSE_MIN_COST = 0
SVA_FUSE_MAX_MARGIN = 1
SVA_FUSE_MEDIAN = 2      # sva_array_depth_conf and sva_array_depth_sub only
SVA_ARRAY_PAIRS = 0      # sva_array_depth_sub's routes
SVA_ARRAY_GROUPS = 1
SVA_ARRAY_GROUPS_MIXED = 2
SVA_MULTI_GATHER_RCCL = 0
SVA_MULTI_GATHER_PEER = 1
SVA_MULTI_GATHER_ALL = 2


class SgmParams(ct.Structure):
    """Mirror of ``sva_sgm_params`` (include/sva.h)."""
    _fields_ = [
        ("D", ct.c_int32), ("dmin", ct.c_int32), ("dir", ct.c_int32),
        ("P1", ct.c_int32), ("P2", ct.c_int32), ("subpixel", ct.c_int32),
        ("lr_check", ct.c_int32), ("lr_max_diff", ct.c_int32),
        ("invalid", ct.c_uint16), ("_pad", ct.c_uint16), ("dir_y", ct.c_int32),
    ]


class RectifyView(ct.Structure):
    """Mirror of ``sva_rectify_view`` (include/sva.h): h, the row-major 3x3 from a
    rectified pixel to the undistorted raw pixel; the raw camera's cx, cy, fx, fy;
    the Brown-Conrady coefficients k1, k2, p1, p2, k3."""
    _fields_ = [("h", ct.c_double * 9), ("cx", ct.c_double), ("cy", ct.c_double),
                ("fx", ct.c_double), ("fy", ct.c_double), ("k1", ct.c_double),
                ("k2", ct.c_double), ("p1", ct.c_double), ("p2", ct.c_double),
                ("k3", ct.c_double)]

    @classmethod
    def make(cls, h=(1, 0, 0, 0, 1, 0, 0, 0, 1), cx=0.0, cy=0.0, fx=1.0, fy=1.0, dist=(0,) * 5):
        return cls((ct.c_double * 9)(*[float(v) for v in np.asarray(h).ravel()]), cx, cy, fx, fy,
                   *[float(v) for v in dist])


class Camera(ct.Structure):
    """Mirror of ``sva_camera`` = class Camera (include/Camera.h:6-21)."""
    _fields_ = [("f", ct.c_double), ("pos", ct.c_double * 3), ("pixel_size", ct.c_double)]

    @classmethod
    def make(cls, f, pos, pixel_size):
        c = cls()
        c.f = f
        c.pos[0], c.pos[1], c.pos[2] = pos
        c.pixel_size = pixel_size
        return c


class TileLayout(ct.Structure):
    """Mirror of ``sva_tile_layout`` (include/sva.h): the tile stages' buffers."""
    _fields_ = [("seg", ct.c_int32), ("nsx", ct.c_int32), ("nsy", ct.c_int32),
                ("diag_volumes", ct.c_int32),
                ("cost_bytes", ct.c_size_t), ("diag_bytes", ct.c_size_t),
                ("hckpt_bytes", ct.c_size_t), ("vckpt_bytes", ct.c_size_t)]


class FrameLayout(ct.Structure):
    """Mirror of ``sva_frame_layout`` (include/sva.h): the frame plan's buffers."""
    _fields_ = [("route", ct.c_int32), ("minima", ct.c_int32), ("D", ct.c_int32),
                ("seg", ct.c_int32), ("nsx", ct.c_int32), ("nsy", ct.c_int32),
                ("n_volumes", ct.c_int32), ("reserved", ct.c_int32),
                ("cost_bytes", ct.c_size_t), ("volumes_bytes", ct.c_size_t),
                ("ckpt_bytes", ct.c_size_t),
                ("hck_off", ct.c_size_t), ("hck_bytes", ct.c_size_t),
                ("vck_off", ct.c_size_t), ("vck_bytes", ct.c_size_t),
                ("pair_off", ct.c_size_t), ("pair_bytes", ct.c_size_t),
                ("hmn_off", ct.c_size_t), ("hmn_bytes", ct.c_size_t),
                ("vmn_off", ct.c_size_t), ("vmn_bytes", ct.c_size_t)]


class PairJob(ct.Structure):
    _fields_ = [
        ("left", ct.c_void_p), ("right", ct.c_void_p), ("width", ct.c_int32),
        ("height", ct.c_int32), ("pitch", ct.c_size_t), ("disp", ct.c_void_p),
        ("subpix", ct.c_void_p),
    ]


class PairD(ct.Structure):
    """sva_pair_d: one device-resident pair for sva_batch_sgm_d."""
    _fields_ = [("left", ct.c_void_p), ("right", ct.c_void_p), ("params", SgmParams)]


class ArrayPair(ct.Structure):
    """sva_array_pair: one camera-array pair for sva_array_depth."""
    _fields_ = [("ref", ct.c_int32), ("other", ct.c_int32), ("params", SgmParams),
                ("baseline", ct.c_double)]


class SvaError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"sva status {status}: {msg}")
        self.status = status


def _preload_single_hip_runtime() -> None:
    """Keep ONE HIP runtime per process.  PyTorch-ROCm wheels bundle their own
    libamdhip64 (same SONAME as /opt/rocm's).  If libsva.so were loaded first it
    would bind /opt/rocm's copy and a later `import torch` would map a second
    runtime whose device init then fails.  Preloading torch's copy by path makes
    libsva.so (and torch, whenever imported) bind that single runtime."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        ct.CDLL(cand, mode=ct.RTLD_GLOBAL)


def _load() -> ct.CDLL:
    _preload_single_hip_runtime()
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback)")
    lib = ct.CDLL(LIB_PATH)
    vp, i32, sz, dbl = ct.c_void_p, ct.c_int, ct.c_size_t, ct.c_double
    P = ct.POINTER
    # the entries that take a route: the frame (ctx .. n_groups), then route .. cost_second;
    # the chain's entries add one argument group per stage
    frame = [vp, P(vp), i32, i32, i32, sz, P(ArrayPair), i32, P(i32), i32]
    routed = frame + [i32, P(dbl), dbl, dbl, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    check_tail = [P(ct.c_int32), i32, i32, i32, i32, vp, vp]
    speckle_tail = [i32, i32, i32, vp]
    fill_tail = [i32, i32, i32, vp]
    wmed_tail = [i32, vp, i32, i32, vp]
    rect_tail = [P(RectifyView), i32, i32, vp, vp]
    rectify = [vp, vp, i32, i32, i32, sz, P(RectifyView), i32, i32, sz, i32, vp, vp, vp]
    mask = [vp, vp, vp, i32, i32, i32, vp, ct.c_uint16, vp, vp]
    sig = {
        "sva_sgm_params_default": (None, [P(SgmParams)]),
        "sva_abi_version": (i32, []),
        "sva_device_count": (i32, [P(i32)]),
        "sva_create": (i32, [i32, P(vp)]),
        "sva_destroy": (i32, [vp]),
        "sva_set_stream": (i32, [vp, vp]),
        "sva_synchronize": (i32, [vp]),
        "sva_last_error": (ct.c_char_p, [vp]),
        "sva_status_string": (ct.c_char_p, [i32]),
        "sva_reserve": (i32, [vp, i32, i32, i32]),
        "sva_set_path_kernel": (i32, [vp, i32]),
        "sva_set_timing": (i32, [vp, i32]),
        "sva_reset_timing": (i32, [vp]),
        "sva_kernel_time": (i32, [vp, ct.c_char_p, P(dbl), P(ct.c_int64)]),
        "sva_set_debug": (i32, [vp, i32, ct.c_int64]),
        "sva_get_debug": (i32, [vp, i32, P(ct.c_int64)]),
        "sva_disparity_sgm": (i32, [vp, vp, vp, i32, i32, sz, P(SgmParams), vp, vp]),
        "sva_disparity_sgm_d": (i32, [vp, vp, vp, i32, i32, sz, P(SgmParams), vp, vp]),
        "sva_disparity_sgm_conf": (i32, [vp, vp, vp, i32, i32, sz, P(SgmParams), i32, vp, vp, vp,
                                         vp]),
        "sva_disparity_sgm_conf_d": (i32, [vp, vp, vp, i32, i32, sz, P(SgmParams), i32, vp, vp,
                                           vp, vp]),
        "sva_wta_conf_d": (i32, [vp, vp, i32, i32, P(SgmParams), i32, vp, vp, vp, vp]),
        "sva_fuse_depth_conf_d": (i32, [vp, vp, vp, vp, i32, i32, i32, P(dbl), dbl, dbl,
                                        ct.c_uint16, i32, vp, vp, vp]),
        "sva_fuse_depth_conf": (i32, [vp, vp, vp, vp, i32, i32, i32, P(dbl), dbl, dbl,
                                      ct.c_uint16, i32, vp, vp, vp]),
        "sva_census_d": (i32, [vp, vp, i32, i32, sz, vp]),
        "sva_cost_d": (i32, [vp, vp, vp, i32, i32, P(SgmParams), vp]),
        "sva_paths_d": (i32, [vp, vp, i32, i32, P(SgmParams), vp]),
        "sva_census_cost_d": (i32, [vp, vp, vp, i32, i32, sz, P(SgmParams), vp]),
        "sva_aggregate_d": (i32, [vp, vp, i32, i32, P(SgmParams), vp]),
        "sva_wta_d": (i32, [vp, vp, i32, i32, P(SgmParams), vp, vp]),
        "sva_tile_layout_of": (i32, [i32, i32, i32, P(TileLayout)]),
        "sva_tile_check": (i32, [i32, i32, i32, sz, sz, sz, sz]),
        "sva_paths_tile_d": (i32, [vp, vp, sz, i32, i32, P(SgmParams), vp, sz, vp, sz, vp, sz]),
        "sva_wta_hv_d": (i32, [vp, vp, sz, vp, sz, vp, sz, vp, sz, i32, i32, P(SgmParams), vp,
                               vp]),
        "sva_frame_layout_of": (i32, [i32, i32, P(SgmParams), ct.c_longlong, P(FrameLayout)]),
        "sva_paths_frame_d": (i32, [vp, vp, sz, i32, i32, P(SgmParams), vp, sz, vp, sz]),
        "sva_wta_frame_d": (i32, [vp, vp, sz, vp, sz, vp, sz, i32, i32, P(SgmParams), i32, vp, vp,
                                  vp, vp]),
        "sva_disparity_ref": (i32, [vp, vp, vp, i32, i32, sz, vp, P(Camera), P(Camera), i32,
                                    dbl, dbl, vp, vp, vp]),
        "sva_disparity_ref_d": (i32, [vp, vp, vp, i32, i32, sz, vp, P(Camera), P(Camera), i32,
                                      dbl, dbl, vp, vp, vp]),
        "sva_ref_endpoints_d": (i32, [vp, i32, i32, P(Camera), P(Camera), i32, dbl, dbl, vp, vp]),
        "sva_disparity_to_depth_d": (i32, [vp, vp, i32, dbl, dbl, dbl, vp]),
        "sva_disparity_to_depth": (i32, [vp, vp, i32, dbl, dbl, dbl, vp]),
        "sva_fuse_depth_d": (i32, [vp, vp, i32, i32, i32, P(dbl), dbl, dbl, ct.c_uint16, vp, vp]),
        "sva_fuse_depth": (i32, [vp, vp, i32, i32, i32, P(dbl), dbl, dbl, ct.c_uint16, vp, vp]),
        "sva_shift_perspective_d": (i32, [vp, P(Camera), P(Camera), vp, vp, i32, i32, sz, vp]),
        "sva_shift_perspective": (i32, [vp, P(Camera), P(Camera), vp, vp, i32, i32, sz, vp]),
        "sva_improve_with_disparity_d": (i32, [vp, vp, vp, P(vp), P(Camera), i32, i32, i32, sz,
                                               vp, i32, i32, vp]),
        "sva_improve_with_disparity": (i32, [vp, vp, vp, P(vp), P(Camera), i32, i32, i32, sz,
                                             vp, i32, i32, vp]),
        "sva_shift_perspective2_d": (i32, [vp, P(Camera), P(Camera), vp, i32, i32, vp]),
        "sva_shift_perspective2": (i32, [vp, P(Camera), P(Camera), vp, i32, i32, vp]),
        "sva_points_to_depth_d": (i32, [vp, vp, ct.c_int64, P(Camera), i32, i32, vp]),
        "sva_points_to_depth": (i32, [vp, vp, ct.c_int64, P(Camera), i32, i32, vp]),
        "sva_depth_to_points_d": (i32, [vp, vp, i32, i32, P(Camera), vp, P(ct.c_int64)]),
        "sva_depth_to_points": (i32, [vp, vp, i32, i32, P(Camera), vp, P(ct.c_int64)]),
        "sva_resize_half_size": (i32, [i32, i32, P(i32), P(i32)]),
        "sva_resize_half_d": (i32, [vp, vp, i32, i32, sz, vp, sz]),
        "sva_resize_half": (i32, [vp, vp, i32, i32, sz, vp, sz]),
        "sva_batch_sgm": (i32, [P(vp), i32, P(PairJob), i32, P(SgmParams), P(i32)]),
        "sva_multi_create": (i32, [P(i32), i32, i32, i32, P(vp)]),
        "sva_multi_destroy": (i32, [vp]),
        "sva_multi_synchronize": (i32, [vp]),
        "sva_multi_last_error": (ct.c_char_p, [vp]),
        "sva_multi_plan": (i32, [i32, i32, i32, P(i32), P(i32), P(i32)]),
        "sva_multi_context": (i32, [vp, i32, i32, P(vp)]),
        "sva_batch_sgm_d": (i32, [vp, P(PairD), i32, i32, i32, sz, vp, vp]),
        "sva_disparity_sgm_batch_d": (i32, [vp, P(PairD), i32, i32, i32, sz, vp, vp]),
        "sva_array_depth": (i32, [vp, P(vp), i32, i32, i32, sz, P(ArrayPair), i32, P(i32), i32,
                                  dbl, dbl, vp, vp, vp]),
        "sva_disparity_sgm_batch_conf_d": (i32, [vp, P(PairD), i32, i32, i32, sz, i32, vp, vp, vp,
                                                 vp]),
        "sva_batch_sgm_conf_d": (i32, [vp, P(PairD), i32, i32, i32, sz, i32, vp, vp, vp, vp]),
        "sva_array_depth_conf": (i32, [vp, P(vp), i32, i32, i32, sz, P(ArrayPair), i32, P(i32),
                                       i32, dbl, dbl, i32, i32, vp, vp, vp, vp, vp, vp]),
        "sva_cost_fuse_d": (i32, [vp, vp, sz, i32, i32, i32, i32, i32, i32, P(ct.c_int32), vp]),
        "sva_disparity_sgm_multi": (i32, [vp, vp, P(vp), P(ct.c_int32), i32, i32, i32, sz,
                                          P(SgmParams), i32, vp, vp, vp, vp]),
        "sva_disparity_sgm_multi_d": (i32, [vp, vp, P(vp), P(ct.c_int32), i32, i32, i32, sz,
                                            P(SgmParams), i32, vp, vp, vp, vp]),
        "sva_array_depth_mb": (i32, [vp, P(vp), i32, i32, i32, sz, P(ArrayPair), i32, P(i32), i32,
                                     dbl, dbl, i32, vp, vp, vp, vp]),
        "sva_cost_mixed_d": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
        "sva_cost_fuse_mixed_d": (i32, [vp, vp, sz, i32, i32, i32, i32, i32, i32, P(ct.c_int32),
                                        P(ct.c_int32), vp]),
        "sva_disparity_sgm_mixed": (i32, [vp, vp, P(vp), P(ct.c_int32), P(ct.c_int32), i32, i32,
                                          i32, sz, P(SgmParams), i32, vp, vp, vp, vp]),
        "sva_disparity_sgm_mixed_d": (i32, [vp, vp, P(vp), P(ct.c_int32), P(ct.c_int32), i32, i32,
                                            i32, sz, P(SgmParams), i32, vp, vp, vp, vp]),
        "sva_array_depth_mixed": (i32, [vp, P(vp), i32, i32, i32, sz, P(ArrayPair), i32, P(i32),
                                        i32, P(dbl), dbl, dbl, i32, vp, vp, vp, vp]),
        "sva_fuse_depth_sub_d": (i32, [vp, vp, vp, i32, i32, i32, P(dbl), dbl, dbl, ct.c_uint16, vp,
                                       vp]),
        "sva_fuse_depth_sub": (i32, [vp, vp, vp, i32, i32, i32, P(dbl), dbl, dbl, ct.c_uint16, vp,
                                     vp]),
        "sva_fuse_depth_conf_sub_d": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, P(dbl), dbl, dbl,
                                            ct.c_uint16, i32, vp, vp, vp]),
        "sva_fuse_depth_conf_sub": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, P(dbl), dbl, dbl,
                                          ct.c_uint16, i32, vp, vp, vp]),
        "sva_array_depth_sub": (i32, routed),
        "sva_cross_check_d": (i32, [vp, vp, vp, i32, i32, i32, P(ct.c_int32), ct.c_uint16, i32, i32,
                                    i32, vp, vp, vp, vp]),
        "sva_cross_check": (i32, [vp, vp, vp, i32, i32, i32, P(ct.c_int32), ct.c_uint16, i32, i32,
                                  i32, vp, vp, vp, vp]),
        "sva_array_depth_checked": (i32, routed + check_tail),
        "sva_filter_speckles_d": (i32, [vp, vp, vp, i32, i32, i32, ct.c_uint16, i32, i32, vp, vp,
                                        vp]),
        "sva_filter_speckles": (i32, [vp, vp, vp, i32, i32, i32, ct.c_uint16, i32, i32, vp, vp, vp]),
        "sva_array_depth_filtered": (i32, routed + check_tail + speckle_tail),
        "sva_fill_holes_d": (i32, [vp, vp, vp, i32, i32, i32, ct.c_uint16, i32, i32, i32, vp, vp, vp]),
        "sva_fill_holes": (i32, [vp, vp, vp, i32, i32, i32, ct.c_uint16, i32, i32, i32, vp, vp, vp]),
        "sva_array_depth_filled": (i32, routed + check_tail + speckle_tail + fill_tail),
        "sva_array_depth_smoothed": (i32, routed + check_tail + speckle_tail + fill_tail +
                                     wmed_tail),
        "sva_array_depth_rectified": (i32, routed + check_tail + speckle_tail + fill_tail +
                                      wmed_tail + rect_tail),
        "sva_rectify_d": (i32, rectify),
        "sva_rectify": (i32, rectify),
        "sva_rectify_view_of": (i32, [P(dbl), P(dbl), P(dbl), P(dbl), P(RectifyView)]),
        "sva_mask_maps_d": (i32, mask),
        "sva_mask_maps": (i32, mask),
        "sva_weighted_median_d": (i32, [vp, vp, vp, vp, sz, vp, vp, i32, i32, i32, ct.c_uint16, i32,
                                        i32, i32, vp, vp, vp]),
        "sva_weighted_median": (i32, [vp, vp, vp, vp, sz, vp, vp, i32, i32, i32, ct.c_uint16, i32,
                                      i32, i32, vp, vp, vp]),
        "sva_resize_linear_f64_d": (i32, [vp, vp, i32, i32, vp, i32, i32]),
        "sva_resize_linear_f64": (i32, [vp, vp, i32, i32, vp, i32, i32]),
        "sva_ref_error_d": (i32, [vp, vp, i32, i32, vp, i32, i32, ct.c_double, vp]),
        "sva_ref_error": (i32, [vp, vp, i32, i32, vp, i32, i32, ct.c_double, vp]),
        "sva_masked_mean_d": (i32, [vp, vp, vp, i32, i32, P(ct.c_double)]),
        "sva_masked_mean": (i32, [vp, vp, vp, i32, i32, P(ct.c_double)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    # a stale build exports the same symbols with other semantics: refuse it
    have = lib.sva_abi_version()
    if have != ABI_VERSION:
        raise ImportError(f"{LIB_PATH} implements ABI v{have}, this binding needs v{ABI_VERSION}: "
                          "rebuild it (python -c 'import __graft_entry__ as g; g.build()')")
    return lib


lib = _load()


def wmed_weights(sigma) -> np.ndarray:
    """The weight table of the weighted median filter for an
    intensity scale sigma > 0: 256 u16, entry i = round(1024 * exp(-i / sigma))
    (sva.hpp's wmedWeights)."""
    if not sigma > 0:
        raise ValueError("sigma must be positive")
    return np.floor(1024.0 * np.exp(-np.arange(256) / float(sigma)) + 0.5).astype(np.uint16)


def rectify_view(K_raw, dist, R, K_ideal) -> RectifyView:
    """sva_rectify_view_of: the view of a calibration, h = K_raw .
    R . K_ideal^-1 with R taking ideal-camera rays to raw-camera rays; dist = (k1,
    k2, p1, p2, k3).  Host only."""
    def arr(a, n):
        a = np.ascontiguousarray(a, dtype=np.float64).ravel()
        if a.size != n:
            raise ValueError(f"expected {n} values")
        return (ct.c_double * n)(*a)
    out = RectifyView()
    st = lib.sva_rectify_view_of(arr(K_raw, 9), arr(dist, 5), arr(R, 9), arr(K_ideal, 9),
                                 ct.byref(out))
    if st != SVA_OK:
        raise SvaError(st, "sva_rectify_view_of")
    return out


def _view_table(rect):
    """A sequence of RectifyView as a C array (one is passed through); None stays
    a null pointer."""
    if rect is None or isinstance(rect, ct.Array):
        return rect
    return (RectifyView * max(1, len(rect)))(*rect)


def default_params(**kw) -> SgmParams:
    p = SgmParams()
    lib.sva_sgm_params_default(ct.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def resize_half_size(W: int, H: int):
    """Output size of the ingestion resize: (cvRound(W/2), cvRound(H/2))."""
    dw, dh = ct.c_int(0), ct.c_int(0)
    if lib.sva_resize_half_size(W, H, ct.byref(dw), ct.byref(dh)) != 0:
        raise ValueError("bad size")
    return dw.value, dh.value


def tile_layout(W: int, H: int, D: int) -> TileLayout:
    """Plane sizes of the tile stages (sva_tile_layout_of; no device needed)."""
    out = TileLayout()
    st = lib.sva_tile_layout_of(W, H, D, ct.byref(out))
    if st != SVA_OK:
        raise SvaError(st, "sva_tile_layout_of")
    return out


def frame_layout(W: int, H: int, params: SgmParams, pair_min_pixels: int = -1) -> FrameLayout:
    """The plan a frame of this shape and these penalties runs (sva_frame_layout_of;
    no device needed).  pair_min_pixels = -1: the built-in pair-route threshold."""
    out = FrameLayout()
    st = lib.sva_frame_layout_of(W, H, ct.byref(params), pair_min_pixels, ct.byref(out))
    if st != SVA_OK:
        raise SvaError(st, "sva_frame_layout_of")
    return out


def device_count() -> int:
    n = ct.c_int(0)
    lib.sva_device_count(ct.byref(n))
    return n.value


def _ptr(a) -> int | None:
    if a is None:
        return None
    if isinstance(a, int):
        return a
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return a.data_ptr()  # torch tensor


def _i32_pairs(pairs):
    """A list of (a, b) as a C [n][2] i32 array; None stays a null pointer."""
    if pairs is None:
        return None
    return (ct.c_int32 * max(2, 2 * len(pairs)))(*[int(v) for s in pairs for v in s])


def _steps(view_step, n):
    """n (x, y) view positions as a C [n][2] i32 array (a short list is padded
    with zeros, so that the library's own checks see it); None stays null."""
    if view_step is None:
        return None
    flat = [int(v) for s in view_step for v in s]
    return (ct.c_int32 * max(2, 2 * n, len(flat)))(*flat)


def _ptr_table(arrays):
    """The data pointers of a list of arrays as a C array."""
    return (ct.c_void_p * max(1, len(arrays)))(*[_ptr(a) for a in arrays])


def _pair_table(pairs):
    """A list of (left_ptr, right_ptr, SgmParams) as a C sva_pair_d array."""
    jobs = (PairD * len(pairs))()
    for i, (l, r, p) in enumerate(pairs):
        jobs[i] = PairD(_ptr(l), _ptr(r), p)
    return jobs


class _ArrayFrame:
    """The C form of one array frame (sva_array_depth*).  images: HxW u8 views;
    pairs: (ref, other, SgmParams, baseline) each; group_start: G + 1 offsets.
    head: the arguments from `images` to `n_groups`."""

    def __init__(self, images, pairs, group_start):
        self.imgs = [np.ascontiguousarray(a, dtype=np.uint8) for a in images]
        self.H, self.W = self.imgs[0].shape
        self.P, self.G = len(pairs), len(group_start) - 1
        jp = (ArrayPair * self.P)()
        for i, (a, b, p, base) in enumerate(pairs):
            jp[i] = ArrayPair(a, b, p, base)
        self.head = (_ptr_table(self.imgs), len(self.imgs), self.W, self.H, self.W, jp, self.P,
                     (ct.c_int32 * len(group_start))(*group_start), self.G)

    def planes(self, n, dtype, want=True):
        """An [n, H, W] output, or None for one not asked for."""
        return np.zeros((n, self.H, self.W), dtype) if want else None


class Context:
    """One device + one stream (``sva_create``)."""

    def __init__(self, device: int = 0):
        h = ct.c_void_p()
        st = lib.sva_create(device, ct.byref(h))
        if st != SVA_OK:
            raise SvaError(st, lib.sva_status_string(st).decode())
        self.h = h
        self.device = device
        self._owned = True

    @classmethod
    def borrowed(cls, handle: int, device: int):
        """A non-owning view of a context another owner destroys (e.g. one of
        a Multi engine's, sva_multi_context)."""
        c = cls.__new__(cls)
        c.h = ct.c_void_p(handle)
        c.device = device
        c._owned = False
        return c

    def close(self):
        if self.h and self._owned:
            lib.sva_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, st: int):
        if st != SVA_OK:
            raise SvaError(st, lib.sva_last_error(self.h).decode())

    # -- plumbing
    def set_stream(self, stream_ptr: int | None):
        self._chk(lib.sva_set_stream(self.h, stream_ptr))

    def synchronize(self):
        self._chk(lib.sva_synchronize(self.h))

    def reserve(self, W, H, D):
        self._chk(lib.sva_reserve(self.h, W, H, D))

    def set_path_kernel(self, kernel: int):
        self._chk(lib.sva_set_path_kernel(self.h, kernel))

    def set_timing(self, on):
        """on: False/True, SVA_TIMING_PATHS (the path kernel only) or SVA_TIMING_AGG
        (the path kernel and wta_hv, the two aggregation kernels)."""
        self._chk(lib.sva_set_timing(self.h, int(on)))

    def reset_timing(self):
        self._chk(lib.sva_reset_timing(self.h))

    def set_debug(self, key: int, value: int):
        """sva_set_debug: SVA_DEBUG_PLANE_SPLIT / SVA_DEBUG_FAIL_COST_AT (tests),
        SVA_DEBUG_PLACEMENT_TRIALS (sva_reserve's placement check),
        SVA_DEBUG_REFINE_ROUTE (1 = the refinement's box-sum route at every k >= 1)."""
        self._chk(lib.sva_set_debug(self.h, key, int(value)))

    def get_debug(self, key: int) -> int:
        v = ct.c_int64(0)
        self._chk(lib.sva_get_debug(self.h, key, ct.byref(v)))
        return v.value

    def kernel_time(self, name: str) -> tuple[float, int]:
        ms = ct.c_double(0)
        n = ct.c_int64(0)
        self._chk(lib.sva_kernel_time(self.h, name.encode(), ct.byref(ms), ct.byref(n)))
        return ms.value, n.value

    # -- Mode S, host arrays
    def disparity_sgm(self, left: np.ndarray, right: np.ndarray, params: SgmParams):
        assert left.dtype == np.uint8 and right.dtype == np.uint8 and left.shape == right.shape
        left = np.ascontiguousarray(left)
        right = np.ascontiguousarray(right)
        H, W = left.shape
        disp = np.zeros((H, W), np.uint16)
        sub = np.zeros((H, W), np.float32) if params.subpixel else None
        self._chk(lib.sva_disparity_sgm(self.h, _ptr(left), _ptr(right), W, H, W,
                                        ct.byref(params), _ptr(disp), _ptr(sub)))
        return disp, sub

    # -- Mode S, device pointers (async on the context stream)
    def disparity_sgm_d(self, left, right, W, H, pitch, params, disp, sub=None):
        self._chk(lib.sva_disparity_sgm_d(self.h, _ptr(left), _ptr(right), W, H, pitch,
                                          ct.byref(params), _ptr(disp), _ptr(sub)))

    # -- Mode S with the WTA's confidence planes and the uniqueness filter
    def disparity_sgm_conf(self, left: np.ndarray, right: np.ndarray, params: SgmParams,
                           uniqueness: int = 0):
        """(disp, sub, cost_min, cost_second): sva_disparity_sgm_conf.  cost_min =
        S(d*), cost_second = min S(d) over |d - d*| > 1 (0xFFFF if none);
        uniqueness = u in 0..100 rejects pixels with cost_second * (100 - u) <
        cost_min * 100 (disp = params.invalid, sub = NaN)."""
        assert left.dtype == np.uint8 and right.dtype == np.uint8 and left.shape == right.shape
        left = np.ascontiguousarray(left)
        right = np.ascontiguousarray(right)
        H, W = left.shape
        disp = np.zeros((H, W), np.uint16)
        sub = np.zeros((H, W), np.float32) if params.subpixel else None
        cmin = np.zeros((H, W), np.uint16)
        csec = np.zeros((H, W), np.uint16)
        self._chk(lib.sva_disparity_sgm_conf(self.h, _ptr(left), _ptr(right), W, H, W,
                                             ct.byref(params), int(uniqueness), _ptr(disp),
                                             _ptr(sub), _ptr(cmin), _ptr(csec)))
        return disp, sub, cmin, csec

    def disparity_sgm_conf_d(self, left, right, W, H, pitch, params, uniqueness, disp, sub=None,
                             cost_min=None, cost_second=None):
        self._chk(lib.sva_disparity_sgm_conf_d(self.h, _ptr(left), _ptr(right), W, H, pitch,
                                               ct.byref(params), int(uniqueness), _ptr(disp),
                                               _ptr(sub), _ptr(cost_min), _ptr(cost_second)))

    # -- multi-baseline Mode S: one reference image, n matched images,
    # -- and its mixed-baseline form: pairs of unequal baselines in one volume (§2.2d).
    # `ratios` below is () or (the C ratio table,): the one argument the mixed calls add
    def _sgm_multi_d(self, fn, ref, others, steps, ratios, W, H, pitch, params, uniqueness, disp,
                     sub, cost_min, cost_second):
        self._chk(fn(self.h, _ptr(ref), _ptr_table(others), _i32_pairs(steps), *ratios,
                     len(others), W, H, pitch, ct.byref(params), int(uniqueness), _ptr(disp),
                     _ptr(sub), _ptr(cost_min), _ptr(cost_second)))

    def _sgm_multi(self, fn, ref, others, steps, ratios, params, uniqueness):
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        oth = [np.ascontiguousarray(a, dtype=np.uint8) for a in others]
        assert len(oth) == len(steps) and all(a.shape == ref.shape for a in oth)
        H, W = ref.shape
        disp = np.zeros((H, W), np.uint16)
        sub = np.zeros((H, W), np.float32) if params.subpixel else None
        cmin = np.zeros((H, W), np.uint16)
        csec = np.zeros((H, W), np.uint16)
        self._sgm_multi_d(fn, ref, oth, steps, ratios, W, H, W, params, uniqueness, disp, sub,
                          cmin, csec)
        return disp, sub, cmin, csec

    def disparity_sgm_multi(self, ref: np.ndarray, others, steps, params: SgmParams,
                            uniqueness: int = 0):
        """(disp, sub, cost_min, cost_second): sva_disparity_sgm_multi.  others: n
        HxW u8 images, steps: n (dir, dir_y) steps; the n cost volumes are fused
        (mean over the pairs whose matched pixel is inside the image) before one
        aggregation.  params.dir / dir_y are ignored."""
        return self._sgm_multi(lib.sva_disparity_sgm_multi, ref, others, steps, (), params,
                               uniqueness)

    def disparity_sgm_multi_d(self, ref, others, steps, W, H, pitch, params, uniqueness, disp,
                              sub=None, cost_min=None, cost_second=None):
        """Device pointers; others: n image pointers, steps: n (dir, dir_y)."""
        self._sgm_multi_d(lib.sva_disparity_sgm_multi_d, ref, others, steps, (), W, H, pitch,
                          params, uniqueness, disp, sub, cost_min, cost_second)

    def cost_fuse_d(self, volumes, stride, steps, W, H, D, dreal, dmin, fused):
        """sva_cost_fuse_d: len(steps) device volumes [H][W][D] u8, `stride` bytes
        apart, fused into `fused`."""
        self._chk(lib.sva_cost_fuse_d(self.h, _ptr(volumes), stride, len(steps), W, H, D, dreal,
                                      dmin, _i32_pairs(steps), _ptr(fused)))

    def disparity_sgm_mixed(self, ref: np.ndarray, others, steps, ratios, params: SgmParams,
                            uniqueness: int = 0):
        """(disp, sub, cost_min, cost_second): sva_disparity_sgm_mixed.  As
        disparity_sgm_multi, with ratios: n (num, den) -- pair i's major-axis
        baseline over the group's unit baseline, each in 1..8 (None = a null
        pointer, which the library refuses)."""
        return self._sgm_multi(lib.sva_disparity_sgm_mixed, ref, others, steps,
                               (_i32_pairs(ratios),), params, uniqueness)

    def disparity_sgm_mixed_d(self, ref, others, steps, ratios, W, H, pitch, params, uniqueness,
                              disp, sub=None, cost_min=None, cost_second=None):
        """Device pointers; others: n image pointers, steps: n (dir, dir_y),
        ratios: n (num, den)."""
        self._sgm_multi_d(lib.sva_disparity_sgm_mixed_d, ref, others, steps,
                          (_i32_pairs(ratios),), W, H, pitch, params, uniqueness, disp, sub,
                          cost_min, cost_second)

    def cost_mixed_d(self, census_ref, census_oth, W, H, D, dreal, dmin, step, ratio, C):
        """sva_cost_mixed_d: the cost volume [H][W][D] u8 of one pair at ratio =
        (num, den) of the unit baseline along step = (sx, sy), from two device
        census maps."""
        self._chk(lib.sva_cost_mixed_d(self.h, _ptr(census_ref), _ptr(census_oth), W, H, D, dreal,
                                       dmin, int(step[0]), int(step[1]), int(ratio[0]),
                                       int(ratio[1]), _ptr(C)))

    def cost_fuse_mixed_d(self, volumes, stride, steps, ratios, W, H, D, dreal, dmin, fused):
        """sva_cost_fuse_mixed_d: cost_fuse_d with volume i visible by the rule of
        a pair at ratios[i] = (num, den)."""
        self._chk(lib.sva_cost_fuse_mixed_d(self.h, _ptr(volumes), stride, len(steps), W, H, D,
                                            dreal, dmin, _i32_pairs(steps), _i32_pairs(ratios),
                                            _ptr(fused)))


    def wta_conf_d(self, S, W, H, params, uniqueness, disp, sub=None, cost_min=None,
                   cost_second=None):
        self._chk(lib.sva_wta_conf_d(self.h, _ptr(S), W, H, ct.byref(params), int(uniqueness),
                                     _ptr(disp), _ptr(sub), _ptr(cost_min), _ptr(cost_second)))

    def disparity_sgm_batch_d(self, pairs, W, H, pitch, maps, sub=None):
        """pairs: list of (left_ptr, right_ptr, SgmParams) on this context's device;
        maps: [n][H][W] u16 device, sub: [n][H][W] f32 device or None."""
        self._chk(lib.sva_disparity_sgm_batch_d(self.h, _pair_table(pairs), len(pairs), W, H,
                                                pitch, _ptr(maps), _ptr(sub)))

    def disparity_sgm_batch_conf_d(self, pairs, W, H, pitch, uniqueness, maps, sub=None,
                                   cost_min=None, cost_second=None):
        """disparity_sgm_batch_d through the confidence instance: cost_min /
        cost_second are [n][H][W] u16 device planes or None; the pairs also
        share params.invalid."""
        self._chk(lib.sva_disparity_sgm_batch_conf_d(self.h, _pair_table(pairs), len(pairs), W, H,
                                                     pitch, int(uniqueness), _ptr(maps), _ptr(sub),
                                                     _ptr(cost_min), _ptr(cost_second)))


    def census_d(self, img, W, H, pitch, out):
        self._chk(lib.sva_census_d(self.h, _ptr(img), W, H, pitch, _ptr(out)))

    def cost_d(self, cl, cr, W, H, params, C):
        self._chk(lib.sva_cost_d(self.h, _ptr(cl), _ptr(cr), W, H, ct.byref(params), _ptr(C)))

    def paths_d(self, C, W, H, params, L8):
        self._chk(lib.sva_paths_d(self.h, _ptr(C), W, H, ct.byref(params), _ptr(L8)))

    def census_cost_d(self, left, right, W, H, pitch, params, C):
        self._chk(lib.sva_census_cost_d(self.h, _ptr(left), _ptr(right), W, H, pitch,
                                        ct.byref(params), _ptr(C)))

    def aggregate_d(self, C, W, H, params, S):
        self._chk(lib.sva_aggregate_d(self.h, _ptr(C), W, H, ct.byref(params), _ptr(S)))

    def paths_tile_d(self, C, C_bytes, W, H, params, diag, diag_bytes, hck, hck_bytes, vck,
                     vck_bytes):
        self._chk(lib.sva_paths_tile_d(self.h, _ptr(C), C_bytes, W, H, ct.byref(params),
                                       _ptr(diag), diag_bytes, _ptr(hck), hck_bytes, _ptr(vck),
                                       vck_bytes))

    def wta_hv_d(self, C, C_bytes, diag, diag_bytes, hck, hck_bytes, vck, vck_bytes, W, H, params,
                 disp, sub=None):
        self._chk(lib.sva_wta_hv_d(self.h, _ptr(C), C_bytes, _ptr(diag), diag_bytes, _ptr(hck),
                                   hck_bytes, _ptr(vck), vck_bytes, W, H, ct.byref(params),
                                   _ptr(disp), _ptr(sub)))

    def paths_frame_d(self, C, C_bytes, W, H, params, volumes, volumes_bytes, ckpt, ckpt_bytes):
        self._chk(lib.sva_paths_frame_d(self.h, _ptr(C), C_bytes, W, H, ct.byref(params),
                                        _ptr(volumes), volumes_bytes, _ptr(ckpt), ckpt_bytes))

    def wta_frame_d(self, C, C_bytes, volumes, volumes_bytes, ckpt, ckpt_bytes, W, H, params,
                    uniqueness, disp, sub=None, cost_min=None, cost_second=None):
        self._chk(lib.sva_wta_frame_d(self.h, _ptr(C), C_bytes, _ptr(volumes), volumes_bytes,
                                      _ptr(ckpt), ckpt_bytes, W, H, ct.byref(params),
                                      int(uniqueness), _ptr(disp), _ptr(sub), _ptr(cost_min),
                                      _ptr(cost_second)))

    def wta_d(self, S, W, H, params, disp, sub=None):
        self._chk(lib.sva_wta_d(self.h, _ptr(S), W, H, ct.byref(params), _ptr(disp), _ptr(sub)))

    # -- Mode R
    def disparity_ref(self, ref: np.ndarray, other: np.ndarray, cref: Camera, coth: Camera,
                      k: int = 20, t_near: float = 0.5, t_far: float = 1.0, mask=None,
                      disp_u8=None, disp_u16=None, valid=None):
        ref = np.ascontiguousarray(ref)
        other = np.ascontiguousarray(other)
        H, W = ref.shape
        if disp_u8 is None:
            disp_u8 = np.zeros((H, W), np.uint8)
        if disp_u16 is None:
            disp_u16 = np.zeros((H, W), np.uint16)
        if valid is None:
            valid = np.zeros((H, W), np.uint8)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        self._chk(lib.sva_disparity_ref(self.h, _ptr(ref), _ptr(other), W, H, W, _ptr(m),
                                        ct.byref(cref), ct.byref(coth), k, t_near, t_far,
                                        _ptr(disp_u8), _ptr(disp_u16), _ptr(valid)))
        return disp_u8, disp_u16, valid

    def disparity_ref_d(self, ref, other, W, H, pitch, mask, cref, coth, k, t_near, t_far,
                        disp_u8, disp_u16=None, valid=None):
        self._chk(lib.sva_disparity_ref_d(self.h, _ptr(ref), _ptr(other), W, H, pitch, _ptr(mask),
                                          ct.byref(cref), ct.byref(coth), k, t_near, t_far,
                                          _ptr(disp_u8), _ptr(disp_u16), _ptr(valid)))

    def ref_endpoints_d(self, W, H, cref, coth, k, t_near, t_far, ends, valid):
        self._chk(lib.sva_ref_endpoints_d(self.h, W, H, ct.byref(cref), ct.byref(coth), k,
                                          t_near, t_far, _ptr(ends), _ptr(valid)))

    # -- refinement / 3-D, host arrays
    def shift_perspective(self, cin: Camera, cout: Camera, disp, image, init=None):
        disp = np.ascontiguousarray(disp, dtype=np.uint8)
        image = np.ascontiguousarray(image, dtype=np.uint8)
        H, W = disp.shape
        out = np.zeros((H, W), np.uint8) if init is None else np.array(init, np.uint8)
        self._chk(lib.sva_shift_perspective(self.h, ct.byref(cin), ct.byref(cout), _ptr(disp),
                                            _ptr(image), W, H, W, _ptr(out)))
        return out

    def improve_with_disparity(self, disp, center, images, cam_pairs, window=21, mask=None,
                               strict=False, init=None):
        disp = np.ascontiguousarray(disp, dtype=np.uint8)
        center = np.ascontiguousarray(center, dtype=np.uint8)
        H, W = disp.shape
        imgs = [np.ascontiguousarray(i, dtype=np.uint8) for i in images]
        ptrs = (ct.c_void_p * max(1, len(imgs)))(*[i.ctypes.data for i in imgs])
        cams = (Camera * max(1, 2 * len(cam_pairs)))()
        for i, (a, b) in enumerate(cam_pairs):
            cams[2 * i], cams[2 * i + 1] = a, b
        out = np.zeros((H, W), np.uint8) if init is None else np.array(init, np.uint8)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        self._chk(lib.sva_improve_with_disparity(self.h, _ptr(disp), _ptr(center), ptrs, cams,
                                                 len(imgs), W, H, W, _ptr(m), window,
                                                 int(strict), _ptr(out)))
        return out

    def improve_with_disparity_d(self, disp, center, images, cam_pairs, W, H, pitch, mask,
                                 window, strict, out):
        ptrs = (ct.c_void_p * max(1, len(images)))(*images)
        cams = (Camera * max(1, 2 * len(cam_pairs)))()
        for i, (a, b) in enumerate(cam_pairs):
            cams[2 * i], cams[2 * i + 1] = a, b
        self._chk(lib.sva_improve_with_disparity_d(self.h, _ptr(disp), _ptr(center), ptrs, cams,
                                                   len(images), W, H, pitch, _ptr(mask), window,
                                                   int(strict), _ptr(out)))

    def shift_perspective2(self, cin: Camera, cout: Camera, depth, init=None):
        depth = np.ascontiguousarray(depth, dtype=np.float64)
        H, W = depth.shape
        out = np.zeros((H, W), np.float64) if init is None else np.array(init, np.float64)
        self._chk(lib.sva_shift_perspective2(self.h, ct.byref(cin), ct.byref(cout), _ptr(depth),
                                             W, H, _ptr(out)))
        return out

    def points_to_depth(self, points, cam: Camera, W, H, init=None):
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        out = np.zeros((H, W), np.float64) if init is None else np.array(init, np.float64)
        self._chk(lib.sva_points_to_depth(self.h, _ptr(pts), pts.shape[0], ct.byref(cam), W, H,
                                          _ptr(out)))
        return out

    def depth_to_points(self, depth, cam: Camera):
        depth = np.ascontiguousarray(depth, dtype=np.float64)
        H, W = depth.shape
        pts = np.zeros((W * H, 3), np.float64)
        n = ct.c_int64(0)
        self._chk(lib.sva_depth_to_points(self.h, _ptr(depth), W, H, ct.byref(cam), _ptr(pts),
                                          ct.byref(n)))
        return pts[:n.value].copy()

    def depth_to_points_d(self, depth, W, H, cam: Camera, points) -> int:
        n = ct.c_int64(0)
        self._chk(lib.sva_depth_to_points_d(self.h, _ptr(depth), W, H, ct.byref(cam),
                                            _ptr(points), ct.byref(n)))
        return n.value

    # -- ingestion
    def resize_half(self, img):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        H, W = img.shape
        dw, dh = resize_half_size(W, H)
        out = np.zeros((dh, dw), np.uint8)
        self._chk(lib.sva_resize_half(self.h, _ptr(img), W, H, W, _ptr(out), max(1, dw)))
        return out

    def resize_half_d(self, src, W, H, pitch, dst, dst_pitch):
        self._chk(lib.sva_resize_half_d(self.h, _ptr(src), W, H, pitch, _ptr(dst), dst_pitch))

    # ---- evaluation (CameraStereoVision.cpp:107-119) ----
    def resize_linear(self, src, dw: int, dh: int):
        """resize(src, dst, Size(dw, dh)) INTER_LINEAR on a f64 matrix."""
        src = np.ascontiguousarray(src, dtype=np.float64)
        sh, sw = src.shape
        out = np.zeros((dh, dw), np.float64)
        self._chk(lib.sva_resize_linear_f64(self.h, _ptr(src), sw, sh, _ptr(out), dw, dh))
        return out

    def resize_linear_d(self, src, sw, sh, dst, dw, dh):
        self._chk(lib.sva_resize_linear_f64_d(self.h, _ptr(src), sw, sh, _ptr(dst), dw, dh))

    def ref_error(self, depth, ref, scale: float = 50.0):
        """(resize(depth, ref.size()) - ref) * scale, as the reference's
        ``Mat error = (depth2 - ref) * 50``."""
        depth = np.ascontiguousarray(depth, dtype=np.float64)
        ref = np.ascontiguousarray(ref, dtype=np.float64)
        h, w = depth.shape
        rh, rw = ref.shape
        out = np.zeros((rh, rw), np.float64)
        self._chk(lib.sva_ref_error(self.h, _ptr(depth), w, h, _ptr(ref), rw, rh, scale,
                                    _ptr(out)))
        return out

    def ref_error_d(self, depth, w, h, ref, rw, rh, scale, error):
        self._chk(lib.sva_ref_error_d(self.h, _ptr(depth), w, h, _ptr(ref), rw, rh, scale,
                                      _ptr(error)))

    def masked_mean(self, image, mask=None) -> float:
        """cv::mean(image, mask)[0] (calculateAverageError, functions.cpp:348-354)."""
        image = np.ascontiguousarray(image, dtype=np.float64)
        h, w = image.shape
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        out = ct.c_double(0)
        self._chk(lib.sva_masked_mean(self.h, _ptr(image), _ptr(m), w, h, ct.byref(out)))
        return out.value

    def masked_mean_d(self, image, mask, w, h) -> float:
        out = ct.c_double(0)
        self._chk(lib.sva_masked_mean_d(self.h, _ptr(image), _ptr(mask), w, h, ct.byref(out)))
        return out.value

    def _fuse_d(self, fn, planes, n_maps, W, H, baselines, f, pixel_size, invalid, mode, outs):
        """One sva_fuse_depth* call: planes and outs (arrays, pointers or None) in
        that entry's order; mode None for a median entry, which takes none."""
        b = (ct.c_double * max(1, n_maps))(*[float(v) for v in baselines])
        self._chk(fn(self.h, *map(_ptr, planes), n_maps, W, H, b, f, pixel_size, invalid,
                     *([] if mode is None else [int(mode)]), *map(_ptr, outs)))

    def _fuse(self, fn, disps, planes, baselines, f, pixel_size, invalid, mode, want):
        """The host-array form: planes, (array or None, dtype) pairs shaped as
        disps, follow it in the call; want: whether n_valid (and winner) are
        asked for.  Returns (depth, n_valid[, winner]), None where not wanted."""
        d = np.ascontiguousarray(disps, dtype=np.uint16)
        N, H, W = d.shape
        ins = [d] + [None if x is None else np.ascontiguousarray(x, dtype=t) for x, t in planes]
        assert all(x is None or x.shape == d.shape for x in ins)
        outs = [np.zeros((H, W), np.float64)]
        outs += [np.zeros((H, W), np.uint8) if w else None for w in want]
        self._fuse_d(fn, ins, N, W, H, baselines, f, pixel_size, invalid, mode, outs)
        return tuple(outs)

    def fuse_depth(self, disps: np.ndarray, baselines, f, pixel_size, invalid=0xFFFF):
        return self._fuse(lib.sva_fuse_depth, disps, [], baselines, f, pixel_size, invalid, None,
                          [True])

    def fuse_depth_d(self, disps, n_maps, W, H, baselines, f, pixel_size, invalid, depth,
                     n_valid=None):
        self._fuse_d(lib.sva_fuse_depth_d, [disps], n_maps, W, H, baselines, f, pixel_size,
                     invalid, None, [depth, n_valid])

    def fuse_depth_conf(self, disps: np.ndarray, cost_min: np.ndarray, cost_second, baselines,
                        f, pixel_size, invalid=0xFFFF, mode=SVA_FUSE_MIN_COST):
        """(depth, n_valid, winner): sva_fuse_depth_conf, the depth of the valid
        map with the smallest cost_min (SVA_FUSE_MIN_COST; cost_second may be
        None) or the largest cost_second - cost_min (SVA_FUSE_MAX_MARGIN)."""
        return self._fuse(lib.sva_fuse_depth_conf, disps,
                          [(cost_min, np.uint16), (cost_second, np.uint16)], baselines, f,
                          pixel_size, invalid, mode, [True, True])

    def fuse_depth_conf_d(self, disps, cost_min, cost_second, n_maps, W, H, baselines, f,
                          pixel_size, invalid, mode, depth, n_valid=None, winner=None):
        self._fuse_d(lib.sva_fuse_depth_conf_d, [disps, cost_min, cost_second], n_maps, W, H,
                     baselines, f, pixel_size, invalid, mode, [depth, n_valid, winner])

    def fuse_depth_sub(self, disps: np.ndarray, subpix, baselines, f, pixel_size,
                       invalid=0xFFFF, want_n_valid=True):
        """(depth, n_valid or None): sva_fuse_depth_sub, the median of the depths
        of the f32 sub-pixel maps (a map counts where its u16 disparity is valid
        and subpix > 0).  subpix None: the NULL pointer the call refuses."""
        return self._fuse(lib.sva_fuse_depth_sub, disps, [(subpix, np.float32)], baselines, f,
                          pixel_size, invalid, None, [want_n_valid])

    def fuse_depth_sub_d(self, disps, subpix, n_maps, W, H, baselines, f, pixel_size, invalid,
                         depth, n_valid=None):
        self._fuse_d(lib.sva_fuse_depth_sub_d, [disps, subpix], n_maps, W, H, baselines, f,
                     pixel_size, invalid, None, [depth, n_valid])

    def fuse_depth_conf_sub(self, disps: np.ndarray, subpix, cost_min: np.ndarray, cost_second,
                            baselines, f, pixel_size, invalid=0xFFFF, mode=SVA_FUSE_MIN_COST,
                            want_n_valid=True, want_winner=True):
        """(depth, n_valid, winner): sva_fuse_depth_conf_sub, fuse_depth_conf with
        the winner's depth taken from its f32 sub-pixel map."""
        return self._fuse(lib.sva_fuse_depth_conf_sub, disps,
                          [(subpix, np.float32), (cost_min, np.uint16), (cost_second, np.uint16)],
                          baselines, f, pixel_size, invalid, mode, [want_n_valid, want_winner])

    def fuse_depth_conf_sub_d(self, disps, subpix, cost_min, cost_second, n_maps, W, H, baselines,
                              f, pixel_size, invalid, mode, depth, n_valid=None, winner=None):
        self._fuse_d(lib.sva_fuse_depth_conf_sub_d, [disps, subpix, cost_min, cost_second], n_maps,
                     W, H, baselines, f, pixel_size, invalid, mode, [depth, n_valid, winner])

    @staticmethod
    def _filter_maps(disps, subpix):
        """What the four map filters' host forms share: (d, s, N, H, W, out, osub) --
        the [N][H][W] u16 maps and f32 maps (or None) as C arrays, and zeroed outputs
        of their shapes."""
        d = np.ascontiguousarray(disps, dtype=np.uint16)
        s = None if subpix is None else np.ascontiguousarray(subpix, dtype=np.float32)
        N, H, W = d.shape
        assert s is None or s.shape == d.shape
        return d, s, N, H, W, np.zeros_like(d), None if s is None else np.zeros_like(s)

    def cross_check(self, disps: np.ndarray, view_step, subpix=None, invalid=0xFFFF, max_diff=1,
                    min_agree=1, max_conflict=0, want_agree=True, want_conflict=True):
        """(out, out_sub or None, agree, conflict): sva_cross_check, the cross-view
        consistency check of n maps [n][H][W] u16 of one unit
        baseline; view_step: n (x, y) positions in unit baselines.  A pixel stays
        where at least min_agree other views agree within max_diff and at most
        max_conflict see through it; out_sub (with subpix) is NaN where rejected."""
        d, s, N, H, W, out, osub = self._filter_maps(disps, subpix)
        ag = np.zeros(d.shape, np.uint8) if want_agree else None
        cf = np.zeros(d.shape, np.uint8) if want_conflict else None
        self._chk(lib.sva_cross_check(self.h, _ptr(d), _ptr(s), N, W, H, _steps(view_step, N),
                                      invalid, int(max_diff), int(min_agree), int(max_conflict),
                                      _ptr(out), _ptr(osub), _ptr(ag), _ptr(cf)))
        return out, osub, ag, cf

    def cross_check_d(self, disps, subpix, n_views, W, H, view_step, invalid, max_diff, min_agree,
                      max_conflict, out, out_sub=None, agree=None, conflict=None):
        self._chk(lib.sva_cross_check_d(self.h, _ptr(disps), _ptr(subpix), n_views, W, H,
                                        _steps(view_step, n_views), invalid, int(max_diff),
                                        int(min_agree), int(max_conflict), _ptr(out),
                                        _ptr(out_sub), _ptr(agree), _ptr(conflict)))

    def filter_speckles(self, disps: np.ndarray, max_size, max_diff, subpix=None, invalid=0xFFFF,
                        want_size=True):
        """(out, out_sub or None, comp_size or None): sva_filter_speckles, the
        speckle filter of n maps [n][H][W] u16.  A valid pixel
        whose 4-connected component (neighbours within max_diff) has at most
        max_size pixels becomes `invalid`; out_sub (with subpix) is NaN there."""
        d, s, N, H, W, out, osub = self._filter_maps(disps, subpix)
        size = np.zeros(d.shape, np.uint32) if want_size else None
        self._chk(lib.sva_filter_speckles(self.h, _ptr(d), _ptr(s), N, W, H, invalid, int(max_size),
                                          int(max_diff), _ptr(out), _ptr(osub), _ptr(size)))
        return out, osub, size

    def filter_speckles_d(self, disps, subpix, n_maps, W, H, invalid, max_size, max_diff, out,
                          out_sub=None, comp_size=None):
        """sva_filter_speckles_d on device pointers; out may be disps and out_sub subpix."""
        self._chk(lib.sva_filter_speckles_d(self.h, _ptr(disps), _ptr(subpix), n_maps, W, H, invalid,
                                            int(max_size), int(max_diff), _ptr(out), _ptr(out_sub),
                                            _ptr(comp_size)))

    def fill_holes(self, disps: np.ndarray, max_dist, min_found=1, mode=SVA_FILL_SECOND,
                   subpix=None, invalid=0xFFFF, want_found=True):
        """(out, out_sub or None, n_found or None): sva_fill_holes, hole filling
         of n maps [n][H][W] u16.  A hole (0 or `invalid`) with
        at least min_found valid pixels within max_dist steps along the eight
        directions takes the `mode` statistic of them (sorted by value, distance,
        direction); out_sub (with subpix) takes the chosen source's f32 value."""
        d, s, N, H, W, out, osub = self._filter_maps(disps, subpix)
        found = np.zeros(d.shape, np.uint8) if want_found else None
        self._chk(lib.sva_fill_holes(self.h, _ptr(d), _ptr(s), N, W, H, invalid, int(max_dist),
                                     int(min_found), int(mode), _ptr(out), _ptr(osub), _ptr(found)))
        return out, osub, found

    def fill_holes_d(self, disps, subpix, n_maps, W, H, invalid, max_dist, min_found, mode, out,
                     out_sub=None, n_found=None):
        """sva_fill_holes_d on device pointers; out may be disps and out_sub subpix."""
        self._chk(lib.sva_fill_holes_d(self.h, _ptr(disps), _ptr(subpix), n_maps, W, H, invalid,
                                       int(max_dist), int(min_found), int(mode), _ptr(out),
                                       _ptr(out_sub), _ptr(n_found)))

    def weighted_median(self, disps: np.ndarray, radius, guides=None, weights=None, subpix=None,
                        select=None, min_support=1, fill=1, invalid=0xFFFF, want_support=True):
        """(out, out_sub or None, support or None): sva_weighted_median, the
        weighted median filter of n maps [n][H][W] u16.  guides:
        n u8 images [H][W] (views are passed with their row stride), weights: 256
        u16 (wmed_weights); both None for the plain median over the valid pixels.
        A considered pixel (select, fill) with at least min_support candidates in
        its (2 * radius + 1)^2 window takes their lower weighted median; out_sub
        (with subpix) takes the source pixel's f32 value; support counts the
        candidates."""
        d, s, N, H, W, out, osub = self._filter_maps(disps, subpix)
        sel = None if select is None else np.ascontiguousarray(select, dtype=np.uint8)
        assert sel is None or sel.shape == d.shape
        garr, w, pitch, keep = None, None, 0, []
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.uint16)
            assert w.shape == (256,)
        if guides is not None:
            assert len(guides) == N
            for g in guides:
                assert g.dtype == np.uint8 and g.shape == (H, W) and (W == 1 or g.strides[1] == 1)
                keep.append(g)
            strides = {int(g.strides[0]) for g in keep} if H > 1 else {W}
            if len(strides) != 1 or min(strides) < W:
                keep = [np.ascontiguousarray(g) for g in keep]
                strides = {W}
            pitch = strides.pop()
            garr = (ct.c_void_p * N)(*[g.ctypes.data for g in keep])
        sup = np.zeros(d.shape, np.uint16) if want_support else None
        self._chk(lib.sva_weighted_median(self.h, _ptr(d), _ptr(s), garr, pitch, _ptr(w), _ptr(sel),
                                          N, W, H, invalid, int(radius), int(min_support),
                                          int(fill), _ptr(out), _ptr(osub), _ptr(sup)))
        return out, osub, sup

    def weighted_median_d(self, disps, subpix, guides, guide_pitch, weights, select, n_maps, W, H,
                          invalid, radius, min_support, fill, out, out_sub=None, support=None):
        """sva_weighted_median_d on device pointers; guides: a sequence of n_maps
        device addresses or None, weights: a numpy array of 256 u16 or None."""
        garr = None if guides is None else (ct.c_void_p * len(guides))(*[None if g is None else int(g) for g in guides])
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint16)
        self._chk(lib.sva_weighted_median_d(self.h, _ptr(disps), _ptr(subpix), garr,
                                            int(guide_pitch), _ptr(w), _ptr(select), n_maps, W, H,
                                            invalid, int(radius), int(min_support), int(fill),
                                            _ptr(out), _ptr(out_sub), _ptr(support)))

    def rectify(self, views: np.ndarray, rect, size=None, border=0, want_valid=False,
                want_map=False):
        """(out, valid or None, map or None): sva_rectify of n raw
        views [n][src_h][src_w] u8 by rect, n RectifyView, onto size = (out_w, out_h)
        (None: the source's).  valid [n][out_h][out_w] u8; map [n][out_h][out_w][2]
        i32, the source position in 1/32 px (INT32_MIN where outside)."""
        src = np.ascontiguousarray(views, dtype=np.uint8)
        n, sh, sw = src.shape
        assert len(rect) == n
        W, H = (sw, sh) if size is None else (int(size[0]), int(size[1]))
        out = np.zeros((n, H, W), np.uint8)
        valid = np.zeros((n, H, W), np.uint8) if want_valid else None
        qmap = np.zeros((n, H, W, 2), np.int32) if want_map else None
        self._chk(lib.sva_rectify(self.h, _ptr(src), n, sw, sh, sw, _view_table(rect), W, H, W,
                                  int(border), _ptr(out), _ptr(valid), _ptr(qmap)))
        return out, valid, qmap

    def rectify_d(self, src, n, src_w, src_h, src_pitch, rect, out_w, out_h, out_pitch, border,
                  out, valid=None, map=None):
        """sva_rectify_d on device pointers; rect: a sequence of n RectifyView (host)."""
        self._chk(lib.sva_rectify_d(self.h, _ptr(src), n, src_w, src_h, int(src_pitch),
                                    _view_table(rect), out_w, out_h, int(out_pitch), int(border),
                                    _ptr(out), _ptr(valid), _ptr(map)))

    def mask_maps(self, disps: np.ndarray, valid, invalid=0xFFFF, subpix=None):
        """(out, out_sub or None): sva_mask_maps: n maps [n][H][W]
        u16 take `invalid` -- and out_sub (with subpix) NaN -- where their valid
        plane [n][H][W] u8 is 0."""
        d, s, N, H, W, out, osub = self._filter_maps(disps, subpix)
        v = np.ascontiguousarray(valid, dtype=np.uint8)
        assert v.shape == d.shape
        self._chk(lib.sva_mask_maps(self.h, _ptr(d), _ptr(s), N, W, H, _ptr(v), invalid, _ptr(out),
                                    _ptr(osub)))
        return out, osub

    def mask_maps_d(self, disps, subpix, n_maps, W, H, valid, invalid, out, out_sub=None):
        """sva_mask_maps_d on device pointers; out may be disps and out_sub subpix."""
        self._chk(lib.sva_mask_maps_d(self.h, _ptr(disps), _ptr(subpix), n_maps, W, H, _ptr(valid),
                                      invalid, _ptr(out), _ptr(out_sub)))

    def disparity_to_depth(self, disp: np.ndarray, cam_distance, f, pixel_size):
        d = np.ascontiguousarray(disp, dtype=np.uint8)
        out = np.zeros(d.shape, np.float64)
        self._chk(lib.sva_disparity_to_depth(self.h, _ptr(d), d.size, cam_distance, f, pixel_size,
                                             _ptr(out)))
        return out

    def disparity_to_depth_d(self, disp, n, cam_distance, f, pixel_size, depth):
        self._chk(lib.sva_disparity_to_depth_d(self.h, _ptr(disp), n, cam_distance, f,
                                               pixel_size, _ptr(depth)))


def batch_sgm(contexts: list[Context], pairs: list[tuple[np.ndarray, np.ndarray]],
              params: SgmParams, statuses: list | None = None):
    """Match independent pairs round-robin over ``contexts`` (``sva_batch_sgm``).
    With ``statuses`` (a list), per-pair status codes are appended to it and a
    failing pair does not raise; otherwise the first failure raises."""
    jobs = (PairJob * len(pairs))()
    outs = []
    keep = []
    for i, (l, r) in enumerate(pairs):
        l = np.ascontiguousarray(l)
        r = np.ascontiguousarray(r)
        H, W = l.shape
        d = np.zeros((H, W), np.uint16)
        s = np.zeros((H, W), np.float32) if params.subpixel else None
        keep += [l, r]
        outs.append((d, s))
        jobs[i] = PairJob(_ptr(l), _ptr(r), W, H, W, _ptr(d), _ptr(s))
    hs = (ct.c_void_p * len(contexts))(*[c.h.value for c in contexts])
    js = (ct.c_int * max(1, len(pairs)))()
    st = lib.sva_batch_sgm(hs, len(contexts), jobs, len(pairs), ct.byref(params), js)
    if statuses is not None:
        statuses.extend(js[:len(pairs)])
    elif st != SVA_OK:
        raise SvaError(st, lib.sva_status_string(st).decode())
    return outs


def multi_plan(n_devices: int, streams: int, n_jobs: int):
    """(device_index, context_index, slot_index) arrays of sva_multi_plan."""
    d = np.zeros(max(n_jobs, 1), np.int32)
    c = np.zeros(max(n_jobs, 1), np.int32)
    s = np.zeros(max(n_jobs, 1), np.int32)
    st = lib.sva_multi_plan(n_devices, streams, n_jobs,
                            d.ctypes.data_as(ct.POINTER(ct.c_int32)),
                            c.ctypes.data_as(ct.POINTER(ct.c_int32)),
                            s.ctypes.data_as(ct.POINTER(ct.c_int32)))
    if st != SVA_OK:
        raise SvaError(st, "sva_multi_plan")
    return d[:n_jobs], c[:n_jobs], s[:n_jobs]


class Multi:
    """The multi-GPU engine (sva_multi_*): pairs shard over ``devices`` (pair j
    -> device j mod N, round-robin over ``streams`` contexts per device) and
    the maps are gathered to devices[0] (RCCL or peer copies)."""

    def __init__(self, devices, streams: int = 2, flags: int = SVA_MULTI_GATHER_RCCL):
        self.devices = list(devices)
        arr = (ct.c_int * len(self.devices))(*self.devices)
        self.h = ct.c_void_p()
        st = lib.sva_multi_create(arr, len(self.devices), streams, flags, ct.byref(self.h))
        if st != SVA_OK:
            raise SvaError(st, f"sva_multi_create ({lib.sva_status_string(st).decode()})")

    def close(self):
        if self.h:
            lib.sva_multi_destroy(self.h)
            self.h = ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, st: int):
        if st != SVA_OK:
            raise SvaError(st, lib.sva_multi_last_error(self.h).decode(errors="replace"))

    def synchronize(self):
        self._chk(lib.sva_multi_synchronize(self.h))

    def context_handle(self, device_index: int, stream_index: int) -> int:
        out = ct.c_void_p()
        self._chk(lib.sva_multi_context(self.h, device_index, stream_index, ct.byref(out)))
        return out.value

    def context(self, device_index: int, stream_index: int) -> "Context":
        """The engine's context (device_index, stream_index), borrowed (the
        engine destroys it): kernel timing, or direct per-device calls."""
        return Context.borrowed(self.context_handle(device_index, stream_index),
                                self.devices[device_index])

    def batch_sgm_d(self, pairs, W, H, pitch, maps, sub=None):
        """pairs: list of (left_ptr, right_ptr, SgmParams) on their owner devices."""
        self._chk(lib.sva_batch_sgm_d(self.h, _pair_table(pairs), len(pairs), W, H, pitch,
                                      _ptr(maps), _ptr(sub)))

    def batch_sgm_conf_d(self, pairs, W, H, pitch, uniqueness, maps, sub=None, cost_min=None,
                         cost_second=None):
        """batch_sgm_d with every pair through sva_disparity_sgm_conf_d; cost_min /
        cost_second: [n][H][W] u16 on devices[0] or None (only those given are
        gathered)."""
        self._chk(lib.sva_batch_sgm_conf_d(self.h, _pair_table(pairs), len(pairs), W, H, pitch,
                                           int(uniqueness), _ptr(maps), _ptr(sub), _ptr(cost_min),
                                           _ptr(cost_second)))

    def array_depth_conf(self, images, pairs, group_start, f, pixel_size, uniqueness=0,
                         mode=SVA_FUSE_MIN_COST, want_maps=False, want_costs=False):
        """array_depth with the uniqueness filter on every pair and the fusion
        picked by mode (SVA_FUSE_MIN_COST, SVA_FUSE_MAX_MARGIN, SVA_FUSE_MEDIAN).
        Returns (depth, n_valid, winner [G,H,W] u8 or None with MEDIAN, maps,
        cost_min, cost_second), the last three [P,H,W] u16 or None."""
        fr = _ArrayFrame(images, pairs, group_start)
        depth, nv = fr.planes(fr.G, np.float64), fr.planes(fr.G, np.uint8)
        win = fr.planes(fr.G, np.uint8, mode != SVA_FUSE_MEDIAN)
        maps = fr.planes(fr.P, np.uint16, want_maps)
        cmin, csec = fr.planes(fr.P, np.uint16, want_costs), fr.planes(fr.P, np.uint16, want_costs)
        self._chk(lib.sva_array_depth_conf(self.h, *fr.head, f, pixel_size, int(uniqueness),
                                           int(mode), _ptr(depth), _ptr(nv), _ptr(win), _ptr(maps),
                                           _ptr(cmin), _ptr(csec)))
        return depth, nv, win, maps, cmin, csec

    def _array_depth_groups(self, fn, fr, scale, uniqueness, want_maps, want_costs):
        """The group routes: one map and one pair of cost planes per group.
        scale: the arguments from f to pixel_size."""
        depth = fr.planes(fr.G, np.float64)
        maps = fr.planes(fr.G, np.uint16, want_maps)
        cmin, csec = fr.planes(fr.G, np.uint16, want_costs), fr.planes(fr.G, np.uint16, want_costs)
        self._chk(fn(self.h, *fr.head, *scale, int(uniqueness), _ptr(depth), _ptr(maps),
                     _ptr(cmin), _ptr(csec)))
        return depth, maps, cmin, csec

    def array_depth_mb(self, images, pairs, group_start, f, pixel_size, uniqueness=0,
                       want_maps=False, want_costs=False):
        """The multi-baseline array frame (sva_array_depth_mb): each group's pairs
        (one reference view, equal baselines) are fused at the cost level and
        aggregated once.  Returns (depth [G,H,W] f64, maps, cost_min,
        cost_second), the last three [G,H,W] u16 or None."""
        fr = _ArrayFrame(images, pairs, group_start)
        return self._array_depth_groups(lib.sva_array_depth_mb, fr, (f, pixel_size), uniqueness,
                                        want_maps, want_costs)

    def array_depth_mixed(self, images, pairs, group_start, unit_baseline, f, pixel_size,
                          uniqueness=0, want_maps=False, want_costs=False):
        """sva_array_depth_mixed: array_depth_mb for groups of unequal baselines.
        unit_baseline: one per group; each pair's baseline must be num/den (1..8
        each) of it, and the group's depth is unit_baseline * f / (d * pixel_size)."""
        fr = _ArrayFrame(images, pairs, group_start)
        assert len(unit_baseline) == fr.G
        ub = (ct.c_double * fr.G)(*[float(v) for v in unit_baseline])
        return self._array_depth_groups(lib.sva_array_depth_mixed, fr, (ub, f, pixel_size),
                                        uniqueness, want_maps, want_costs)

    def array_depth_sub(self, images, pairs, group_start, f, pixel_size, route=SVA_ARRAY_PAIRS,
                        unit_baseline=None, uniqueness=0, mode=SVA_FUSE_MEDIAN, want_sub=False,
                        want_maps=False, want_costs=False):
        """sva_array_depth_sub: the frame of array_depth_conf (SVA_ARRAY_PAIRS),
        array_depth_mb (SVA_ARRAY_GROUPS) or array_depth_mixed
        (SVA_ARRAY_GROUPS_MIXED, with unit_baseline) with the depth fused from the
        jobs' f32 sub-pixel maps.  Returns (depth [G,H,W] f64, n_valid, winner,
        subpix [J,H,W] f32, maps, cost_min, cost_second [J,H,W] u16), J = P jobs
        on the pair route and G on the group routes; n_valid is None on the group
        routes, winner there and with MEDIAN, the last four unless asked for."""
        fr = _ArrayFrame(images, pairs, group_start)
        pair = route == SVA_ARRAY_PAIRS
        J = fr.P if pair else fr.G
        ub = None if unit_baseline is None else \
            (ct.c_double * max(1, len(unit_baseline)))(*[float(v) for v in unit_baseline])
        depth = fr.planes(fr.G, np.float64)
        nv = fr.planes(fr.G, np.uint8, pair)
        win = fr.planes(fr.G, np.uint8, pair and mode != SVA_FUSE_MEDIAN)
        sub = fr.planes(J, np.float32, want_sub)
        maps = fr.planes(J, np.uint16, want_maps)
        cmin, csec = fr.planes(J, np.uint16, want_costs), fr.planes(J, np.uint16, want_costs)
        self._chk(lib.sva_array_depth_sub(self.h, *fr.head, int(route), ub, f, pixel_size,
                                          int(uniqueness), int(mode), _ptr(depth), _ptr(nv),
                                          _ptr(win), _ptr(sub), _ptr(maps), _ptr(cmin), _ptr(csec)))
        return depth, nv, win, sub, maps, cmin, csec

    # the planes of the post-filter chain's entries, in the order of their results:
    # name, one per job (else per group), dtype
    _CHAIN_PLANES = (("depth", False, np.float64), ("n_valid", False, np.uint8),
                     ("winner", False, np.uint8), ("subpix", True, np.float32),
                     ("maps", True, np.uint16), ("cost_min", True, np.uint16),
                     ("cost_second", True, np.uint16), ("agree", False, np.uint8),
                     ("conflict", False, np.uint8), ("comp_size", True, np.uint32),
                     ("n_found", True, np.uint8), ("support", True, np.uint16))

    def _array_depth_chain(self, fn, images, pairs, group_start, f, pixel_size, route,
                           unit_baseline, uniqueness, mode, view_step, sub, cross, want, stages=(),
                           extra=()):
        """One call of sva_array_depth_checked, _filtered, _filled or _smoothed.
        cross: (max_diff, min_agree, max_conflict); want: plane name -> asked for,
        for the planes the entry can return besides depth; stages: for each stage
        after the check, its argument group as (the scalars in C order, the name
        of the plane that ends it); extra: the arguments after the last stage.
        Returns the planes as a dict, None where not asked for."""
        fr = _ArrayFrame(images, pairs, group_start)
        # jobs: pairs on the pair route, which only the entries after the check take
        nj = len(pairs) if stages and int(route) == SVA_ARRAY_PAIRS else fr.G
        ub = None if unit_baseline is None else \
            (ct.c_double * max(1, len(unit_baseline)))(*[float(v) for v in unit_baseline])
        vs = None if view_step is None else _steps(view_step, len(view_step))
        want = dict(want, depth=True)
        r = {name: fr.planes(nj if per_job else fr.G, dtype, want[name])
             for name, per_job, dtype in self._CHAIN_PLANES if name in want}
        tail = [_ptr(r.get(name)) for name in ("depth", "n_valid", "winner", "subpix", "maps",
                                               "cost_min", "cost_second")]
        tail += [vs, int(sub), *map(int, cross), _ptr(r["agree"]), _ptr(r["conflict"])]
        for scalars, plane in stages:
            tail += [*scalars, _ptr(r[plane])]
        self._chk(fn(self.h, *fr.head, int(route), ub, f, pixel_size, int(uniqueness), int(mode),
                     *tail, *extra))
        return r

    def array_depth_checked(self, images, pairs, group_start, f, pixel_size, view_step,
                            route=SVA_ARRAY_GROUPS, unit_baseline=None, uniqueness=0, sub=0,
                            max_diff=1, min_agree=1, max_conflict=0, want_sub=False,
                            want_maps=False, want_costs=False, want_counts=False):
        """sva_array_depth_checked: array_depth_mb / array_depth_mixed (sub = 0) or
        the group routes of array_depth_sub (sub = 1) with the cross-view check
         between the groups' maps before depth.  view_step: one
        (x, y) position in unit baselines per image.  Returns (depth [G,H,W] f64,
        subpix [G,H,W] f32, maps, cost_min, cost_second [G,H,W] u16, agree,
        conflict [G,H,W] u8), each but depth None unless asked for; maps, subpix
        and depth are the checked ones."""
        r = self._array_depth_chain(
            lib.sva_array_depth_checked, images, pairs, group_start, f, pixel_size, route,
            unit_baseline, uniqueness, SVA_FUSE_MEDIAN, view_step, sub,
            (max_diff, min_agree, max_conflict),
            dict(subpix=want_sub, maps=want_maps, cost_min=want_costs, cost_second=want_costs,
                 agree=want_counts, conflict=want_counts))
        return tuple(r[k] for k in ("depth", "subpix", "maps", "cost_min", "cost_second", "agree",
                                    "conflict"))

    def array_depth_filtered(self, images, pairs, group_start, f, pixel_size, speckle_max_size,
                             speckle_max_diff, check=0, view_step=None, route=SVA_ARRAY_GROUPS,
                             unit_baseline=None, uniqueness=0, mode=SVA_FUSE_MEDIAN, sub=0,
                             max_diff=1, min_agree=1, max_conflict=0, want_sub=False,
                             want_maps=False, want_costs=False, want_counts=False, want_size=False,
                             want_n_valid=False, want_winner=False):
        """sva_array_depth_filtered: the array frame with the speckle filter
         over every job's map before depth -- after the
        cross-view check with check = 1 (group routes), alone with check = 0 (every
        route; on SVA_ARRAY_PAIRS `mode` fuses each group's filtered maps).
        Returns a dict: depth [G,H,W] f64, and where asked for n_valid, winner
        [G,H,W] u8, subpix f32, maps, cost_min, cost_second u16, comp_size u32
        [jobs,H,W], agree, conflict [G,H,W] u8; None where not."""
        return self._array_depth_chain(
            lib.sva_array_depth_filtered, images, pairs, group_start, f, pixel_size, route,
            unit_baseline, uniqueness, mode, view_step, sub, (max_diff, min_agree, max_conflict),
            dict(n_valid=want_n_valid, winner=want_winner, subpix=want_sub, maps=want_maps,
                 cost_min=want_costs, cost_second=want_costs, agree=want_counts,
                 conflict=want_counts, comp_size=want_size),
            [((int(check), int(speckle_max_size), int(speckle_max_diff)), "comp_size")])

    def array_depth_filled(self, images, pairs, group_start, f, pixel_size, fill_max_dist,
                           fill_min_found=1, fill_mode=SVA_FILL_SECOND, speckle_max_size=0,
                           speckle_max_diff=0, check=0, view_step=None, route=SVA_ARRAY_GROUPS,
                           unit_baseline=None, uniqueness=0, mode=SVA_FUSE_MEDIAN, sub=0,
                           max_diff=1, min_agree=1, max_conflict=0, want_sub=False,
                           want_maps=False, want_costs=False, want_counts=False, want_size=False,
                           want_n_valid=False, want_winner=False, want_found=False):
        """sva_array_depth_filled: array_depth_filtered's frame with hole filling
         over every job's map after the speckle filter and before
        depth.  Returns array_depth_filtered's dict with n_found [jobs,H,W] u8
        added (None unless asked for).  cost_min / cost_second stay the
        matcher's: at a filled pixel they describe the rejected match."""
        return self._array_depth_chain(
            lib.sva_array_depth_filled, images, pairs, group_start, f, pixel_size, route,
            unit_baseline, uniqueness, mode, view_step, sub, (max_diff, min_agree, max_conflict),
            dict(n_valid=want_n_valid, winner=want_winner, subpix=want_sub, maps=want_maps,
                 cost_min=want_costs, cost_second=want_costs, agree=want_counts,
                 conflict=want_counts, comp_size=want_size, n_found=want_found),
            [((int(check), int(speckle_max_size), int(speckle_max_diff)), "comp_size"),
             ((int(fill_max_dist), int(fill_min_found), int(fill_mode)), "n_found")])

    def array_depth_smoothed(self, images, pairs, group_start, f, pixel_size, wmed_radius,
                             wmed_weights=None, wmed_min_support=1, wmed_select=0,
                             fill_max_dist=0, fill_min_found=1, fill_mode=SVA_FILL_SECOND,
                             speckle_max_size=0, speckle_max_diff=0, check=0, view_step=None,
                             route=SVA_ARRAY_GROUPS, unit_baseline=None, uniqueness=0,
                             mode=SVA_FUSE_MEDIAN, sub=0, max_diff=1, min_agree=1, max_conflict=0,
                             want_sub=False, want_maps=False, want_costs=False, want_counts=False,
                             want_size=False, want_n_valid=False, want_winner=False,
                             want_found=False, want_support=False):
        """sva_array_depth_smoothed: array_depth_filled's frame with the weighted
        median filter over every job's map after the fill and
        before depth, guided by the job's reference view (wmed_weights None: the
        unguided median).  wmed_select 0 filters every pixel, 1 only those the fill
        looked at.  Returns array_depth_filled's dict with support [jobs,H,W] u16
        added (None unless asked for)."""
        w = None if wmed_weights is None else np.ascontiguousarray(wmed_weights, dtype=np.uint16)
        assert w is None or w.shape == (256,)
        return self._array_depth_chain(
            lib.sva_array_depth_smoothed, images, pairs, group_start, f, pixel_size, route,
            unit_baseline, uniqueness, mode, view_step, sub, (max_diff, min_agree, max_conflict),
            dict(n_valid=want_n_valid, winner=want_winner, subpix=want_sub, maps=want_maps,
                 cost_min=want_costs, cost_second=want_costs, agree=want_counts,
                 conflict=want_counts, comp_size=want_size,
                 n_found=want_found, support=want_support),
            [((int(check), int(speckle_max_size), int(speckle_max_diff)), "comp_size"),
             ((int(fill_max_dist), int(fill_min_found), int(fill_mode)), "n_found"),
             ((int(wmed_radius), _ptr(w), int(wmed_min_support), int(wmed_select)), "support")])

    def array_depth_rectified(self, raw_views, rect, pairs, group_start, f, pixel_size,
                              wmed_radius=0, wmed_weights=None, wmed_min_support=1, wmed_select=0,
                              fill_max_dist=0, fill_min_found=1, fill_mode=SVA_FILL_SECOND,
                              speckle_max_size=0, speckle_max_diff=0, check=0, view_step=None,
                              route=SVA_ARRAY_GROUPS, unit_baseline=None, uniqueness=0,
                              mode=SVA_FUSE_MEDIAN, sub=0, max_diff=1, min_agree=1,
                              max_conflict=0, border=0, mask=1, want_sub=False, want_maps=False,
                              want_costs=False, want_counts=False, want_size=False,
                              want_n_valid=False, want_winner=False, want_found=False,
                              want_support=False, want_views=False, want_valid=False):
        """sva_array_depth_rectified: array_depth_smoothed's frame from RAW views
        (DESIGN.md §2.5f, §7): every device rectifies the views it needs by rect
        (one RectifyView per view) before its jobs; with mask = 1 every job's map
        is masked by its reference view's valid plane before the cross-view check.
        wmed_radius = 0 switches the weighted median off.  Returns
        array_depth_smoothed's dict with views and valid [n_images,H,W] u8 added
        (None unless asked for; a view no pair names stays zero)."""
        w = None if wmed_weights is None else np.ascontiguousarray(wmed_weights, dtype=np.uint16)
        assert w is None or w.shape == (256,)
        n = len(raw_views)
        H, W = np.asarray(raw_views[0]).shape
        views = np.zeros((n, H, W), np.uint8) if want_views else None
        valid = np.zeros((n, H, W), np.uint8) if want_valid else None
        r = self._array_depth_chain(
            lib.sva_array_depth_rectified, raw_views, pairs, group_start, f, pixel_size, route,
            unit_baseline, uniqueness, mode, view_step, sub, (max_diff, min_agree, max_conflict),
            dict(n_valid=want_n_valid, winner=want_winner, subpix=want_sub, maps=want_maps,
                 cost_min=want_costs, cost_second=want_costs, agree=want_counts,
                 conflict=want_counts, comp_size=want_size,
                 n_found=want_found, support=want_support),
            [((int(check), int(speckle_max_size), int(speckle_max_diff)), "comp_size"),
             ((int(fill_max_dist), int(fill_min_found), int(fill_mode)), "n_found"),
             ((int(wmed_radius), _ptr(w), int(wmed_min_support), int(wmed_select)), "support")],
            extra=(_view_table(rect), int(border), int(mask), _ptr(views), _ptr(valid)))
        r["views"], r["valid"] = views, valid
        return r

    def array_depth(self, images, pairs, group_start, f, pixel_size, want_maps=False):
        """images: list of HxW u8 numpy views; pairs: list of (ref, other,
        SgmParams, baseline); group_start: n_groups + 1 offsets.  Returns
        (depth [G,H,W] f64, n_valid [G,H,W] u8, maps [P,H,W] u16 or None)."""
        fr = _ArrayFrame(images, pairs, group_start)
        depth, nv = fr.planes(fr.G, np.float64), fr.planes(fr.G, np.uint8)
        maps = fr.planes(fr.P, np.uint16, want_maps)
        self._chk(lib.sva_array_depth(self.h, *fr.head, f, pixel_size, _ptr(depth), _ptr(nv),
                                      _ptr(maps)))
        return depth, nv, maps
