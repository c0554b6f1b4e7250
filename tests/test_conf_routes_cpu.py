"""The confidence forms of the batch, engine and array routes at the C-ABI
boundary, without a GPU: declared in include/sva.h, exported by libsva.so,
bound by the Python module, refusing a null context or engine before anything
else, and reachable from include/sva.hpp.  The ABI version stays 6: the three
functions are additive."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sva.h")

NEW = ["sva_disparity_sgm_batch_conf_d", "sva_batch_sgm_conf_d", "sva_array_depth_conf"]


def test_declared_in_header():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert re.search(r"#define\s+SVA_FUSE_MEDIAN\s+2\b", text)


def test_exported_by_library(sva):
    out = subprocess.run(["nm", "-D", "--defined-only", sva.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (sva_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
    assert set(NEW) <= set(sva.EXPORTED)
    assert sva.SVA_FUSE_MEDIAN == 2
    assert (sva.SVA_FUSE_MIN_COST, sva.SVA_FUSE_MAX_MARGIN) == (0, 1)


def test_python_methods_exist(sva):
    assert callable(sva.Context.disparity_sgm_batch_conf_d)
    assert callable(sva.Multi.batch_sgm_conf_d)
    assert callable(sva.Multi.array_depth_conf)


def test_abi_version_unchanged(sva):
    assert sva.ABI_VERSION == 6 == sva.lib.sva_abi_version()


@pytest.mark.parametrize("name", NEW)
def test_null_handle_is_rejected(sva, name):
    fn = getattr(sva.lib, name)
    args = [None] * len(fn.argtypes)
    for i, t in enumerate(fn.argtypes):
        if t not in (sva.ct.c_void_p,) and not hasattr(t, "contents"):
            args[i] = 0
    assert fn(*args) == sva.SVA_ERR_INVALID_ARG


def test_hpp_array_depth_conf_compiles(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text(
        '#include "sva.hpp"\n'
        "std::vector<std::vector<double>> f(sva::MultiEngine& m,\n"
        "        const std::vector<sva::ImageView>& images, const std::vector<sva::Camera>& cams,\n"
        "        const std::vector<std::array<int, 2>>& pairs, const sva_sgm_params& p) {\n"
        "    std::vector<std::vector<uint16_t>> maps;\n"
        "    std::vector<std::vector<uint8_t>> winner;\n"
        "    auto a = sva::computeArrayDepthConf(m, images, cams, pairs, p, 25);\n"
        "    auto b = sva::computeArrayDepthConf(m, images, cams, pairs, p, 0, SVA_FUSE_MEDIAN,\n"
        "                                        0.05, &maps);\n"
        "    auto c = sva::computeArrayDepthConf(m, images, cams, pairs, p, 10,\n"
        "                                        SVA_FUSE_MAX_MARGIN, 0.05, &maps, &winner);\n"
        "    auto d = sva::computeArrayDepth(m, images, cams, pairs, p, 0.05, &maps);\n"
        "    return a.size() + b.size() + c.size() > d.size() ? a : d;\n"
        "}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I",
                    os.path.join(ROOT, "include"), str(src)], check=True)
