"""Mixed-baseline Mode S without a GPU: the new entry points
are declared in include/sva.h, exported by libsva.so, bound by the Python
module, refuse a null handle, and are reachable from include/sva.hpp; the ABI
version stays 6.  csrc/cost_mixed_math.h -- the header the kernels and the host
route compile -- is built into a host program: mixed_lim against the
brute-force inside-count of mixed_expect for every pixel of a small frame,
mixed_distance against Python integers.  The numpy helper itself is pinned to
the oracle at ratio 1/1."""
import os
import re
import subprocess

import numpy as np
import pytest

import mb_expect
import mixed_expect as mx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sva.h")
CSRC = os.path.join(ROOT, "stereovisionarray_amd", "csrc")

NEW = ["sva_cost_mixed_d", "sva_cost_fuse_mixed_d", "sva_disparity_sgm_mixed",
       "sva_disparity_sgm_mixed_d", "sva_array_depth_mixed"]
STEPS = [(1, 0), (-1, 0), (0, 1), (1, 1), (2, -1), (-1, 3), (-3, -2)]
RATIOS = [(1, 1), (2, 1), (3, 1), (8, 1), (1, 2), (1, 8), (2, 3), (3, 2), (7, 8)]
W, H, D = 37, 23, 64


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
    assert callable(sva.Context.disparity_sgm_mixed)
    assert callable(sva.Context.disparity_sgm_mixed_d)
    assert callable(sva.Context.cost_mixed_d)
    assert callable(sva.Context.cost_fuse_mixed_d)
    assert callable(sva.Multi.array_depth_mixed)


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


def test_hpp_mixed_compiles(tmp_path):
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
        "    auto a = sva::computeDisparityMixed(c, ref, images, steps, 2, p);\n"
        "    auto b = sva::computeDisparityMixed(c, ref, images, steps, 1, p, 10, &sub, &cmin, &csec);\n"
        "    auto d = sva::computeArrayDepthMixed(m, images, cams, pairs, p);\n"
        "    auto e = sva::computeArrayDepthMixed(m, images, cams, pairs, p, 1, 10, 0.05, &maps);\n"
        "    return a.size() + b.size() + cmin.size() + d.size() + e.size();\n"
        "}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I",
                    os.path.join(ROOT, "include"), str(src)], check=True)


PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "cost_mixed_math.h"
using namespace sva::mb;
int main(int argc, char** argv) {
    if (argc == 2) {   // the distance: s = 0 .. smax for every num, den in 1..8
        const int smax = std::atoi(argv[1]);
        for (int num = 1; num <= 8; num++)
            for (int den = 1; den <= 8; den++)
                for (int s = 0; s <= smax; s++) std::printf("%d\n", mixed_distance(s, num, den));
        return 0;
    }
    // the limit: W H D dmin sx sy num den -> one lim per pixel, row-major
    const int W = std::atoi(argv[1]), H = std::atoi(argv[2]), D = std::atoi(argv[3]);
    const int dmin = std::atoi(argv[4]), sx = std::atoi(argv[5]), sy = std::atoi(argv[6]);
    const int num = std::atoi(argv[7]), den = std::atoi(argv[8]);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++)
            std::printf("%d\n", mixed_lim(x, y, W, H, sx, sy, num, den, dmin, D));
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("mixedmath")
    src = d / "mixedmath.cpp"
    src.write_text(PROGRAM)
    exe = d / "mixedmath"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o",
                    str(exe)], check=True)
    return str(exe)


def test_distance_equals_python_integers(program):
    """Every s up to 2000 for every num, den in 1..8."""
    smax = 2000
    out = subprocess.run([program, str(smax)], capture_output=True, text=True,
                         check=True).stdout.split()
    got = np.array([int(v) for v in out]).reshape(8, 8, smax + 1)
    for num in range(1, 9):
        for den in range(1, 9):
            exp = [(2 * s * num + den) // (2 * den) for s in range(smax + 1)]
            assert got[num - 1, den - 1].tolist() == exp, (num, den)
            assert np.array_equal(mx.distance(np.arange(smax + 1), num, den), exp)
    # rounded half up, non-decreasing, the identity at 1/1
    assert got[0, 1, :6].tolist() == [0, 1, 1, 2, 2, 3]
    assert (np.diff(got, axis=2) >= 0).all()
    assert got[0, 0].tolist() == list(range(smax + 1))


@pytest.mark.parametrize("dmin", [0, 9])
@pytest.mark.parametrize("num,den", RATIOS)
def test_limit_equals_inside(program, num, den, dmin):
    """in(p, d) is true exactly for d < lim(p): a prefix, and lim is its length."""
    cut, seen = False, False
    for sx, sy in STEPS:
        out = subprocess.run([program] + [str(v) for v in (W, H, D, dmin, sx, sy, num, den)],
                             capture_output=True, text=True, check=True).stdout.split()
        lim = np.array([int(v) for v in out]).reshape(H, W)
        ins = mx.inside(W, H, D, dmin, sx, sy, num, den)
        assert np.array_equal(ins, np.arange(D)[None, None, :] < lim[:, :, None]), (sx, sy)
        assert np.array_equal(lim, ins.sum(axis=2)), (sx, sy)
        cut |= bool((lim < D).any())
        seen |= bool((lim > 0).any())
    # the frame cuts some pixel's range short; at 8/1 from dmin = 9 the first
    # distance, 72, already leaves the 37 x 23 frame: no pixel sees that pair
    assert cut and seen == (mx.distance(dmin, num, den) < max(W, H))


def test_unit_ratio_is_the_equal_baseline_rule():
    for sx, sy in STEPS:
        assert np.array_equal(mx.inside(W, H, D, 9, sx, sy, 1, 1),
                              mb_expect.inside(W, H, D, 9, sx, sy))


def test_helper_cost_at_unit_ratio_equals_the_oracle(oracle):
    rng = np.random.default_rng(77)
    cl = rng.integers(0, 1 << 62, size=(H, W), dtype=np.uint64)
    cr = rng.integers(0, 1 << 62, size=(H, W), dtype=np.uint64)
    for sx, sy in STEPS:
        for dmin in (0, 9):
            assert np.array_equal(mx.cost(cl, cr, D, dmin, sx, sy, 1, 1),
                                  oracle.cost2(cl, cr, D, dmin, sx, sy)), (sx, sy, dmin)
