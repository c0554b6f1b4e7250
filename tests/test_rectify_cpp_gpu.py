"""Build and run tests/cpp/test_rectify.cpp: the C++ mirror of rectification
(include/sva.hpp rectifyViewOf, rectifyViews, maskMaps,
computeArrayDepthRectified) against libsva.so on a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "stereovisionarray_amd")


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpprectify") / "test_rectify")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_rectify.cpp"), "-L", LIBDIR, "-lsva",
                    f"-Wl,-rpath,{LIBDIR}", "-o", out], check=True)
    return out


@pytest.mark.gpu
def test_rectify_mirror_gpu(binary):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rectify mirror ok" in r.stdout
