"""The confidence entry points at the C-ABI boundary, without a GPU: declared
in include/sva.h, exported by libsva.so, and refusing a null context before
anything else.  The ABI version stays 6: the five functions are additive."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sva.h")

NEW = ["sva_disparity_sgm_conf", "sva_disparity_sgm_conf_d", "sva_wta_conf_d",
       "sva_fuse_depth_conf", "sva_fuse_depth_conf_d"]


def test_declared_in_header():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert re.search(r"#define\s+SVA_FUSE_MIN_COST\s+0\b", text)
    assert re.search(r"#define\s+SVA_FUSE_MAX_MARGIN\s+1\b", text)


def test_exported_by_library(sva):
    out = subprocess.run(["nm", "-D", "--defined-only", sva.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (sva_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
    assert set(NEW) <= set(sva.EXPORTED)
    assert (sva.SVA_FUSE_MIN_COST, sva.SVA_FUSE_MAX_MARGIN) == (0, 1)


def test_abi_version_unchanged(sva):
    assert sva.ABI_VERSION == 6 == sva.lib.sva_abi_version()


@pytest.mark.parametrize("name", NEW)
def test_null_context_is_rejected(sva, name):
    fn = getattr(sva.lib, name)
    args = [None] * len(fn.argtypes)
    for i, t in enumerate(fn.argtypes):
        if t not in (sva.ct.c_void_p,) and not hasattr(t, "contents"):
            args[i] = 0
    assert fn(*args) == sva.SVA_ERR_INVALID_ARG
