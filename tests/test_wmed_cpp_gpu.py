"""Build and run tests/cpp/test_wmed.cpp: the C++ mirror of the weighted median
filter (include/sva.hpp wmedWeights, weightedMedian, computeArrayDepthSmoothed)
against libsva.so on a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "stereovisionarray_amd")


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cppwmed") / "test_wmed")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_wmed.cpp"),
                    "-L", LIBDIR, "-lsva", f"-Wl,-rpath,{LIBDIR}", "-o", out], check=True)
    return out


@pytest.mark.gpu
def test_wmed_mirror_gpu(binary):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wmed mirror ok" in r.stdout
