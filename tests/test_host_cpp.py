"""Build and run the C++ host-mirror tests (tests/cpp/test_host.cpp) against
include/sva.hpp + libsva.so."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "stereovisionarray_amd")


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "test_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_host.cpp"),
                    "-L", LIBDIR, "-lsva", f"-Wl,-rpath,{LIBDIR}", "-o", out], check=True)
    return out


def test_host_cpu(binary):
    r = subprocess.run([binary, "cpu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.fixture(scope="module")
def dumped(binary, tmp_path_factory):
    """The mirror's pair tables and bresenham lists (test_host dump)."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_ref_golden as mk
    ends = tmp_path_factory.mktemp("dump") / "endpoints.txt"
    ends.write_text("".join("%d %d %d %d\n" % tuple(r) for r in mk.in_bresenham()))
    r = subprocess.run([binary, "dump", str(ends)], capture_output=True, text=True, check=True)
    return json.loads(r.stdout), mk


def _reference_pairs():
    with open(os.path.join(ROOT, "tests", "golden", "ref_pairs.json")) as f:
        return json.load(f)


def test_pair_tables_equal_the_reference(dumped):
    """reference_quirks = true is the reference's own getCameraPairs (both
    overloads, every pairType, cameraNum 0..24) and getGroups("CHESS")."""
    got, _ = dumped
    ref = _reference_pairs()
    assert len(ref) == 10 + 10 * 25 + 1
    assert got["pairs"] == ref


def test_pair_tables_without_quirks_differ_only_as_documented(dumped):
    """sva.hpp documents two departures for reference_quirks = false, both in
    the per-camera CROSS table: the downward neighbour is cameraNum + 5 where
    the reference has the literal camera 5, and the upward neighbour exists
    from cameraNum - 5 >= 0 (camera 5 gains {5, 0}).  Everything else, the
    CHESS groups included, follows from those two."""
    got, _ = dumped
    ref = _reference_pairs()

    def intended(n, pairs):
        out = [list(p) for p in pairs]
        i = 1 if n - 5 > 0 else 0
        if n + 5 < 25:
            assert out[i] == [n, 5]
            out[i] = [n, n + 5]
        if n == 5:
            out.insert(0, [5, 0])
        return out

    differing = 0
    for g, r in zip(got["pairs_fixed"], ref):
        if r["call"] == "getGroups":
            exp = dict(r, groups=[intended(n, p) for n, p in zip(range(0, 25, 2), r["groups"])])
        elif "cameraNum" in r and r["pairType"] == 5:          # CROSS
            exp = dict(r, pairs=intended(r["cameraNum"], r["pairs"]))
        else:
            exp = r
        assert g == exp
        differing += g != r
    # cameras 1..19 (camera 0's downward neighbour is camera 5 either way), and CHESS
    assert differing == 19 + 1


def test_bresenham_equals_the_reference(dumped):
    got, mk = dumped
    fx = mk.load("ref_bresenham")
    off = fx["offsets"]
    assert len(got["bresenham"]) == len(off) - 1 == len(mk.in_bresenham())
    for i, pts in enumerate(got["bresenham"]):
        assert pts == fx["points"][off[i]:off[i + 1]].tolist(), mk.in_bresenham()[i]


@pytest.mark.gpu
def test_host_gpu(binary):
    r = subprocess.run([binary, "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
