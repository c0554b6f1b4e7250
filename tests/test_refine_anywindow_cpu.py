"""improveWithDisparity without a window cap, the parts that need no device:
the two debug keys of the box-sum route (include/sva.h SVA_DEBUG_REFINE_ROUTE /
SVA_DEBUG_REFINE_LAST_ROUTE) in the header and the binding, the null-context
behaviour of the calls that take them, and the coverage condition of the GPU
module's recipe (tests/test_refine_anywindow_gpu.py) on the CPU oracle."""
import os
import re

import numpy as np

from stereovisionarray_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_debug_keys_exported(sva):
    assert sva.SVA_DEBUG_REFINE_ROUTE == 9
    assert sva.SVA_DEBUG_REFINE_LAST_ROUTE == 10
    hdr = open(os.path.join(ROOT, "include", "sva.h")).read()
    keys = dict(re.findall(r"#define\s+(SVA_DEBUG_\w+)\s+(\d+)", hdr))
    assert keys["SVA_DEBUG_REFINE_ROUTE"] == "9" and keys["SVA_DEBUG_REFINE_LAST_ROUTE"] == "10"
    # every key of the header is mirrored by the binding, no number used twice
    assert len(set(keys.values())) == len(keys)
    for name, val in keys.items():
        assert getattr(sva, name) == int(val)
    assert sva.ABI_VERSION == 6


def test_header_states_no_cap_and_workspace(sva):
    hdr = open(os.path.join(ROOT, "include", "sva.h")).read()
    doc = hdr[hdr.index("improveWithDisparity (functions.cpp:11-52)"):
              hdr.index("int sva_improve_with_disparity_d")]
    assert "<= 32" not in doc
    assert "(width + 1) * (height + 1)" in doc and "sva_destroy" in doc


def test_null_context(sva):
    import ctypes as ct
    assert sva.lib.sva_set_debug(None, sva.SVA_DEBUG_REFINE_ROUTE, 1) == sva.SVA_ERR_INVALID_ARG
    v = ct.c_int64(0)
    assert sva.lib.sva_get_debug(None, sva.SVA_DEBUG_REFINE_LAST_ROUTE, ct.byref(v)) == \
        sva.SVA_ERR_INVALID_ARG
    ptrs = (ct.c_void_p * 1)()
    cams = (sva.Camera * 2)()
    assert sva.lib.sva_improve_with_disparity_d(None, None, None, ptrs, cams, 1, 150, 110, 150,
                                                None, 67, 0, None) == sva.SVA_ERR_INVALID_ARG


def test_oracle_recipe_covers_candidates(oracle):
    """The GPU module's recipe at window 68 (its case with the widest spread):
    each positive direction has at least 5 of the 11 candidates winning
    somewhere, and together all 11."""
    W, H, window, k = 150, 110, 68, 33
    cams = synth.reference_array(0.036 / W)
    rng = np.random.default_rng(window)
    center = synth.texture(H, W, window)
    disp = rng.integers(0, 40, size=(H, W)).astype(np.uint8)
    mask = (rng.random((H, W)) < 0.7).astype(np.uint8)
    seen = set()
    for b, i, (ddx, ddy) in ((11, 0, (1, 0)), (7, 2, (0, 1)), (6, 4, (1, 1))):
        pair = (oracle.OCamera.make(*cams[12]), oracle.OCamera.make(*cams[b]))
        init = np.full((H, W), 200, np.uint8)          # disp - 10 .. disp + 10 never reaches 200
        st, exp = oracle.improve_with_disparity(disp, center, [synth.texture(H, W, 100 + i)],
                                                [pair], window=window, mask=mask, init=init)
        assert st == 0
        wr = np.zeros((H, W), bool)
        wr[k + 5 * ddy:H - k - 5 * ddy + 1, k + 5 * ddx:W - k - 5 * ddx + 1] = mask[
            k + 5 * ddy:H - k - 5 * ddy + 1, k + 5 * ddx:W - k - 5 * ddx + 1] != 0
        assert np.array_equal(exp != 200, wr)          # exactly the masked pixels whose windows fit
        c = (exp[wr].astype(np.int64) - disp[wr] + 128) % 256 - 128
        assert (c % (ddx + ddy) == 0).all()
        won = set((c // (ddx + ddy) + 5).tolist())
        assert won <= set(range(11)) and len(won) >= 5
        seen |= won
    assert seen == set(range(11))
