"""The multi-baseline route without a GPU: the new entry
points are declared in include/sva.h, exported by libsva.so, bound by the
Python module, refuse a null handle, and are reachable from include/sva.hpp;
the ABI version stays 6.  The integer arithmetic of the fusion kernel
(csrc/cost_fuse_math.h, the header cost_fuse.hip compiles) is built into a
host program and checked exhaustively: the division for every n and sum, the
visibility limit against mb_expect.inside for every pixel of a small frame."""
import os
import re
import subprocess

import numpy as np
import pytest

import mb_expect
from test_array_gpu import STEPS_2D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sva.h")
CSRC = os.path.join(ROOT, "stereovisionarray_amd", "csrc")

NEW = ["sva_cost_fuse_d", "sva_disparity_sgm_multi", "sva_disparity_sgm_multi_d",
       "sva_array_depth_mb"]
AXIS_STEPS = [(1, 0), (-1, 0), (0, 1), (0, -1)]


def test_declared_in_header():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name


def test_exported_by_library(sva):
    out = subprocess.run(["nm", "-D", "--defined-only", sva.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (sva_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
    assert set(NEW) <= set(sva.EXPORTED)


def test_python_methods_exist(sva):
    assert callable(sva.Context.cost_fuse_d)
    assert callable(sva.Context.disparity_sgm_multi)
    assert callable(sva.Context.disparity_sgm_multi_d)
    assert callable(sva.Multi.array_depth_mb)


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


def test_hpp_multi_compiles(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text(
        '#include "sva.hpp"\n'
        "size_t f(sva::Engine& c, sva::MultiEngine& m, const sva::ImageView& ref,\n"
        "         const std::vector<sva::ImageView>& images, const std::vector<sva::Camera>& cams,\n"
        "         const std::vector<std::array<int, 2>>& pairs, const sva_sgm_params& p) {\n"
        "    std::vector<sva::PairStep> steps;\n"
        "    for (size_t i = 1; i < cams.size(); i++) steps.push_back(sva::pairStep(cams[0], cams[i]));\n"
        "    std::vector<std::vector<uint16_t>> maps;\n"
        "    std::vector<float> sub;\n"
        "    std::vector<uint16_t> cmin, csec;\n"
        "    auto a = sva::computeDisparityMulti(c, ref, images, steps, p);\n"
        "    auto b = sva::computeDisparityMulti(c, ref, images, steps, p, 10, &sub, &cmin, &csec);\n"
        "    auto d = sva::computeArrayDepthMulti(m, images, cams, pairs, p);\n"
        "    auto e = sva::computeArrayDepthMulti(m, images, cams, pairs, p, 10, 0.05, &maps);\n"
        "    return a.size() + b.size() + cmin.size() + d.size() + e.size();\n"
        "}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I",
                    os.path.join(ROOT, "include"), str(src)], check=True)


PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "cost_fuse_math.h"
using namespace sva::mb;
int main(int argc, char** argv) {
    if (argc == 1) {   // the division: every n, every sum
        long bad = 0, cells = 0;
        for (int n = 1; n <= 32; n++) {
            const unsigned magic = mean_magic(n);
            for (unsigned sum = 0; sum <= 255u * n; sum++, cells++) {
                const unsigned x = 2 * sum + n;
                if (mean_round(x, magic) != x / (2u * n)) bad++;
            }
        }
        std::printf("%ld %ld %u\n", bad, cells, mean_magic(0));
        return 0;
    }
    // the limit: W H D dmin sx sy -> one lim per pixel, row-major
    const int W = std::atoi(argv[1]), H = std::atoi(argv[2]), D = std::atoi(argv[3]);
    const int dmin = std::atoi(argv[4]), sx = std::atoi(argv[5]), sy = std::atoi(argv[6]);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) std::printf("%d\n", pair_lim(x, y, W, H, sx, sy, dmin, D));
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("mbmath")
    src = d / "mbmath.cpp"
    src.write_text(PROGRAM)
    exe = d / "mbmath"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o",
                    str(exe)], check=True)
    return str(exe)


def test_division_is_exact_for_every_n_and_sum(program):
    out = subprocess.run([program], capture_output=True, text=True, check=True).stdout.split()
    bad, cells, magic0 = (int(v) for v in out)
    assert cells == sum(255 * n + 1 for n in range(1, 33))
    assert bad == 0
    assert magic0 == 0


@pytest.mark.parametrize("dmin", [0, 9])
@pytest.mark.parametrize("sx,sy", STEPS_2D + AXIS_STEPS)
def test_limit_equals_inside(program, sx, sy, dmin):
    """in(p, d) is true exactly for d < lim(p): a prefix, and lim is its length."""
    W, H, D = 19, 13, 64
    out = subprocess.run([program] + [str(v) for v in (W, H, D, dmin, sx, sy)],
                         capture_output=True, text=True, check=True).stdout.split()
    lim = np.array([int(v) for v in out]).reshape(H, W)
    ins = mb_expect.inside(W, H, D, dmin, sx, sy)
    assert np.array_equal(ins, np.arange(D)[None, None, :] < lim[:, :, None])
    # the frame is smaller than D: limits inside the range, and pixels with none
    assert lim.max() < D
    if dmin:
        assert (lim == 0).any()
