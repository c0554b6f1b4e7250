"""Hole filling without a GPU.

1. tests/fill_expect.py's numpy form against its plain-Python ray walk, and the
   two worked examples of the rule with their exact counts.
2. csrc/fill_math.h through a host program with its own main, built under
   AddressSanitizer and UBSan and run directly: the sort network against
   std::sort on every order of up to eight keys with absent entries, the pick
   per mode, and the scan's own loop (scan_segment: segments, warm-up, the
   diagonal wrap) over whole small maps, every key, output, count and source
   equal to fill_expect.
3. The rules sva_array_depth_filled adds to check_array_args.
4. The quality table of DESIGN.md §2.5d on tests/cross_scene.py.
Nothing is loaded into Python under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

import cross_scene as cs
import fill_expect as fe
import speckle_expect as se

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereovisionarray_amd", "csrc")
INC = os.path.join(ROOT, "include")
INVALID = 0xFFFF


def build(d, name, text):
    src = d / (name + ".cpp")
    src.write_text(text)
    exe = d / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-g", "-I", CSRC, "-I", INC, str(src), "-o",
                    str(exe)], check=True)
    return str(exe)


def same32(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the expectation itself --------------------------------------------------------
def test_numpy_form_equals_ray_walk():
    """All three modes, every min_found, max_dist in {0, 1, 2, 11}, invalid in
    {0xFFFF, 255, 0}, frames 1x1 .. 12x12."""
    rng = np.random.default_rng(3)
    seen_n, filled_any, left_any = set(), False, False
    for trial in range(240):
        H, W = (int(v) for v in rng.integers(1, 13, 2))
        inv = (0xFFFF, 255, 0)[trial % 3]
        holes = (0.1, 0.5, 0.9, 0.97)[trial // 3 % 4]
        d = fe.random_map(W, H, 1000 + trial, holes=holes, invalid=inv, hi=6)
        if inv == 255:
            d[rng.random((H, W)) < 0.05] = 0xFFFF     # then a disparity like any other
        s = fe.subpix_of(d, trial)
        md = (0, 1, 2, 11)[trial // 12 % 4]
        for mode in fe.MODES:
            for mf in range(1, 9):
                out, osub, nf, filled = fe.fill_holes(d, inv, md, mf, mode, s)
                w_out, w_sub, w_nf, w_filled = fe.walk(d, inv, md, mf, mode, s)
                assert np.array_equal(out, w_out), (trial, mode, mf)
                assert same32(osub, w_sub) and np.array_equal(nf, w_nf)
                assert np.array_equal(filled, w_filled)
                ok = fe.valid(d, inv)
                assert np.array_equal(out[ok], d[ok]) and same32(osub[~filled], s[~filled])
                assert (nf[ok] == 0).all() and np.array_equal(out[~filled], d[~filled])
                if md == 0:
                    assert np.array_equal(out, d) and same32(osub, s) and not nf.any()
                filled_any |= bool(filled.any())
                left_any |= bool((~ok & ~filled & (nf > 0)).any())
        seen_n |= set(nf.ravel().tolist())
    assert seen_n == set(range(9)) and filled_any and left_any


def example_truth():
    """A background plane (4) with a foreground rectangle (10)."""
    t = np.full((24, 40), 4, np.uint16)
    t[EXAMPLE_RECT[0]:EXAMPLE_RECT[1], EXAMPLE_RECT[2]:EXAMPLE_RECT[3]] = 10
    return t


EXAMPLE_RECT = (6, 18, 20, 32)     # y0, y1, x0, x1


def test_worked_example_occlusion_band():
    """A six-pixel hole band left of the foreground and a 3x3 hole in a corner:
    max_dist 8, min_found 1 restores the truth exactly in all three modes."""
    t = example_truth()
    y0, y1, x0, _ = EXAMPLE_RECT
    for hole_value in (0, INVALID):
        d = t.copy()
        d[y0:y1, x0 - 6:x0] = hole_value
        d[:3, :3] = hole_value
        assert (~fe.valid(d, INVALID)).sum() == 6 * (y1 - y0) + 9
        for mode in fe.MODES:
            out, _, nf, filled = fe.fill_holes(d, INVALID, 8, 1, mode)
            assert np.array_equal(out, t), mode
            assert np.array_equal(filled, ~fe.valid(d, INVALID))
            assert np.array_equal(out[fe.valid(d, INVALID)], d[fe.valid(d, INVALID)])
        assert np.array_equal(fe.fill_holes(d, INVALID, 0, 1, fe.MEDIAN)[0], d)


def test_worked_example_random_holes():
    """30 % random holes (default_rng(1)) in that map, max_dist 4, min_found 3:
    MEDIAN restores all 290 holes, SECOND gets 13 wrong and MIN 21."""
    t = example_truth()
    gone = np.random.default_rng(1).random(t.shape) < 0.3
    d = t.copy()
    d[gone] = INVALID
    assert gone.sum() == 290
    wrong = {}
    for mode in fe.MODES:
        out, _, _, filled = fe.fill_holes(d, INVALID, 4, 3, mode)
        assert np.array_equal(out[~gone], t[~gone])      # a valid pixel never changes
        assert np.array_equal(filled, gone)              # every hole finds three candidates
        wrong[mode] = int((out != t).sum())
    assert wrong == {fe.MEDIAN: 0, fe.SECOND: 13, fe.MIN: 21}
    assert np.array_equal(fe.fill_holes(d, INVALID, 0, 3, fe.MEDIAN)[0], d)


# ---- fill_math.h -------------------------------------------------------------------
MATH_PROGRAM = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fill_math.h"
using namespace sva;

#define REQUIRE(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)

// every arrangement of n distinct keys and 8 - n absent entries, n = 0..8
static int sort_network() {
    long long tried = 0;
    for (int n = 0; n <= 8; n++) {
        std::vector<uint32_t> v;
        // keys that differ in d, in j only and in k only
        for (int i = 0; i < n; i++)
            v.push_back(fl::make_key(i < 3 ? 7 : 7 + i / 3, i < 3 ? 2 : 1 + i % 2, i));
        for (int i = n; i < 8; i++) v.push_back(fl::kAbsent);
        std::sort(v.begin(), v.end());
        const std::vector<uint32_t> want = v;
        do {
            uint32_t k[8];
            std::copy(v.begin(), v.end(), k);
            REQUIRE(fl::sort8(k) == n);
            REQUIRE(std::equal(k, k + 8, want.begin()));
            tried++;
        } while (std::next_permutation(v.begin(), v.end()));
    }
    // the 0-1 principle, all 256 inputs
    for (unsigned bits = 0; bits < 256; bits++) {
        uint32_t k[8];
        for (int i = 0; i < 8; i++) k[i] = bits >> i & 1u;
        fl::sort8(k);
        REQUIRE(std::is_sorted(k, k + 8));
    }
    std::printf("arrangements %lld\n", tried);
    return 0;
}

static int picks_and_keys() {
    for (int n = 0; n <= 8; n++)
        for (int mf = 1; mf <= 8; mf++) {
            const bool on = n >= mf;
            REQUIRE(fl::pick(n, mf, 0) == (on ? 0 : -1));
            REQUIRE(fl::pick(n, mf, 1) == (on ? std::min(1, n - 1) : -1));
            REQUIRE(fl::pick(n, mf, 2) == (on ? (n - 1) / 2 : -1));
        }
    for (unsigned d : {1u, 255u, 65535u})
        for (int j : {1, 128, 255})
            for (int k = 0; k < 8; k++) {
                const uint32_t key = fl::make_key(d, j, k);
                REQUIRE(key != fl::kAbsent && fl::key_d(key) == d && fl::key_j(key) == j &&
                        fl::key_k(key) == k);
            }
    REQUIRE(fl::make_key(9, 255, 7) < fl::make_key(10, 1, 0));
    REQUIRE(fl::make_key(9, 3, 7) < fl::make_key(9, 4, 0));
    REQUIRE(!fl::thresholds_error(0, 1, 0) && !fl::thresholds_error(255, 8, 2));
    REQUIRE(fl::thresholds_error(-1, 1, 0) && fl::thresholds_error(256, 1, 0));
    REQUIRE(fl::thresholds_error(1, 0, 0) && fl::thresholds_error(1, 9, 0));
    REQUIRE(fl::thresholds_error(1, 1, -1) && fl::thresholds_error(1, 1, 3));
    return 0;
}

struct Load {
    const std::vector<unsigned>* d;
    int W, H;
    unsigned operator()(int x, int y) const {
        if (x < 0 || x >= W || y < 0 || y >= H) std::abort();   // the walk left the frame
        return (*d)[(size_t)y * W + x];
    }
};
struct Store {
    std::vector<uint32_t>* k;
    std::vector<int>* writes;
    int W, H;
    void operator()(int x, int y, uint32_t key) const {
        if (x < 0 || x >= W || y < 0 || y >= H) std::abort();
        (*k)[(size_t)y * W + x] = key;
        (*writes)[(size_t)y * W + x]++;
    }
};

// cases: W H invalid max_dist min_found mode S, then H * W values.  Per pixel:
// the eight keys, out, n_found, the source index (-1: not filled).
template <int RING>
static int scan_cases(std::FILE* f) {
    int W, H, invalid, md, mf, mode, S;
    while (std::fscanf(f, "%d %d %d %d %d %d %d", &W, &H, &invalid, &md, &mf, &mode, &S) == 7) {
        std::vector<unsigned> d((size_t)W * H);
        for (unsigned& v : d) REQUIRE(std::fscanf(f, "%u", &v) == 1);
        std::vector<std::vector<uint32_t>> keys(8, std::vector<uint32_t>((size_t)W * H, 12345u));
        for (int k = 0; k < 8 && md > 0; k++) {
            std::vector<int> writes((size_t)W * H, 0);
            const int lines = fl::n_lines(k, W, H), segs = fl::n_segments(k, W, H, S);
            for (int seg = segs - 1; seg >= 0; seg--)      // any order: nothing is carried
                for (int line = 0; line < lines; line++)
                    fl::scan_segment<RING>(k, line, seg, W, H, S, md, (unsigned)invalid,
                                           Load{&d, W, H}, Store{&keys[k], &writes, W, H});
            for (int w : writes) REQUIRE(w == 1);          // every pixel's key exactly once
        }
        for (int p = 0; p < W * H; p++) {
            uint32_t k8[8];
            for (int k = 0; k < 8; k++) {
                k8[k] = md > 0 ? keys[k][p] : fl::kAbsent;
                std::printf("%u ", k8[k]);
            }
            unsigned out = d[p];
            int found = 0, src = -1;
            if (!cc::valid(d[p], (unsigned)invalid)) {
                found = fl::sort8(k8);
                const int e = fl::pick(found, mf, mode);
                if (e >= 0) {
                    out = fl::key_d(k8[e]);
                    const int j = fl::key_j(k8[e]), k = fl::key_k(k8[e]);
                    src = p + j * (fl::dir_dy(k) * W + fl::dir_dx(k));
                }
            }
            std::printf("%u %d %d\n", out, found, src);
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 1) {
        if (int s = sort_network()) return s;
        return picks_and_keys();
    }
    if (argc != 3) return 2;
    std::FILE* f = std::fopen(argv[2], "r");
    if (!f) return 2;
    const int ring = std::atoi(argv[1]);
    const int s = ring == 1 ? scan_cases<1>(f) : ring == 3 ? scan_cases<3>(f) : scan_cases<4>(f);
    std::fclose(f);
    return s;
}
"""


@pytest.fixture(scope="module")
def math_exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("fillmath"), "fillmath", MATH_PROGRAM)


def test_sort_network_and_pick(math_exe):
    run = subprocess.run([math_exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    # sum over n of 8! / (8 - n)!
    assert run.stdout.strip() == "arrangements 109601"


def scan_cases():
    """(W, H, invalid, max_dist, min_found, mode, S, map): segment lengths 1, 2, 3
    and longer, max_dist above, at and below them, frames narrower than
    max_dist, one row, one column, one pixel."""
    cases = []
    rng = np.random.default_rng(21)
    frames = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (5, 3), (8, 8), (11, 6), (6, 11), (12, 12)]
    n = 0
    for W, H in frames:
        for S in (1, 2, 3, 5, 64):
            for md in sorted({1, 2, 3, 4, max(W, H) - 1, max(W, H) + 3, 255} - {0}):
                inv = (0xFFFF, 255, 0)[n % 3]
                holes = (0.3, 0.7, 0.95, 1.0, 0.0)[n % 5]
                d = fe.random_map(W, H, 5000 + n, holes=holes, invalid=inv, hi=5)
                cases.append((W, H, inv, md, int(rng.integers(1, 9)) if n % 4 else 1, n % 3, S, d))
                n += 1
    # one valid pixel in each corner and in the centre of an all-hole frame
    for W, H in ((9, 9), (12, 5)):
        for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)):
            d = np.zeros((H, W), np.uint16)
            d[y, x] = 9
            for S, md in ((2, 3), (3, 255), (4, 8)):
                cases.append((W, H, INVALID, md, 1, fe.SECOND, S, d))
    return cases


@pytest.mark.parametrize("ring", [1, 3, 4])
def test_scan_loop_equals_fill_expect(math_exe, tmp_path, ring):
    cases = scan_cases()
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for W, H, inv, md, mf, mode, S, d in cases:
            f.write("%d %d %d %d %d %d %d\n" % (W, H, inv, md, mf, mode, S))
            f.write(" ".join(str(int(v)) for v in d.ravel()) + "\n")
    run = subprocess.run([math_exe, str(ring), str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-400:] + run.stderr
    rows = np.array([[int(v) for v in line.split()] for line in run.stdout.splitlines()],
                    dtype=np.int64)
    assert rows.shape == (sum(c[0] * c[1] for c in cases), 11)
    at = 0
    filled_seen = 0
    for W, H, inv, md, mf, mode, S, d in cases:
        got = rows[at:at + W * H]
        at += W * H
        keys = fe.candidates(d, inv, md)
        assert np.array_equal(got[:, :8].T.reshape(8, H, W), keys), (W, H, md, S)
        s = np.arange(W * H, dtype=np.float32).reshape(H, W)     # subpix = the pixel's index
        out, osub, nf, filled = fe.apply(d, keys, inv, mf, mode, s)
        assert np.array_equal(got[:, 8].reshape(H, W), out), (W, H, md, S, mf, mode)
        assert np.array_equal(got[:, 9].reshape(H, W), nf)
        src = got[:, 10].reshape(H, W)
        assert np.array_equal(src >= 0, filled)
        assert np.array_equal(src[filled], osub[filled].astype(np.int64))
        filled_seen += int(filled.sum())
    assert filled_seen > 1000


# ---- the rules sva_array_depth_filled adds ------------------------------------------
ARGS_PROGRAM = r"""
#include <cstdio>
#include <string>
#include <vector>
#include "array_args.h"
using namespace sva;
int main() {
    const int W = 16, H = 8;
    std::vector<uint8_t> img(W * H);
    const uint8_t* images[2] = {img.data(), img.data()};
    sva_array_pair pair{};
    pair.ref = 0;
    pair.other = 1;
    pair.baseline = 0.05;
    pair.params.D = 64;
    pair.params.dir = -1;
    pair.params.invalid = 0xFFFF;
    const int32_t gs[2] = {0, 1};
    std::vector<double> depth(W * H);
    // {check, speckle_max_size, fill_max_dist, fill_min_found, fill_mode}
    const int rows[][5] = {{0, 0, 0, 1, 0},   {0, 20, 255, 8, 2}, {0, 0, -1, 1, 0}, {0, 0, 256, 1, 0},
                           {0, 0, 4, 0, 0},   {0, 0, 4, 9, 0},    {0, 0, 4, 1, -1}, {0, 0, 4, 1, 3},
                           {0, 0, 256, 0, 3}, {0, 0, 4, 0, 3},    {2, 0, 256, 1, 0}, {0, -1, 256, 1, 0}};
    for (const auto& r : rows) {
        ArrayArgs a;
        a.images = images;
        a.n_images = 2;
        a.W = W;
        a.H = H;
        a.pitch = W;
        a.pairs = &pair;
        a.n_pairs = 1;
        a.group_start = gs;
        a.n_groups = 1;
        a.f = 0.05;
        a.pixel_size = 1e-5;
        a.route = ArrayRoute::Groups;
        a.conf = true;
        a.depth = depth.data();
        a.speckle = true;
        a.check = r[0];
        a.speckle_max_size = r[1];
        a.fill = true;
        a.fill_max_dist = r[2];
        a.fill_min_found = r[3];
        a.fill_mode = r[4];
        std::string msg;
        std::vector<int32_t> ratio;
        const int st = check_array_args(a, msg, ratio);
        std::printf("%d|%s\n", st, msg.c_str());
        // without a.fill the fill's values are not looked at
        a.fill = false;
        const int st0 = check_array_args(a, msg, ratio);
        if (r[0] == 0 && r[1] >= 0 && st0 != SVA_OK) return 1;
    }
    return 0;
}
"""


def test_array_entry_rules(tmp_path):
    exe = build(tmp_path, "fillargs", ARGS_PROGRAM)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    got = [line.split("|") for line in run.stdout.splitlines()]
    dist, found, mode = ("fill max_dist must be 0..255", "fill min_found must be 1..8",
                         "fill mode must be 0..2")
    want = [("0", ""), ("0", ""), ("1", dist), ("1", dist), ("1", found), ("1", found), ("1", mode),
            ("1", mode), ("1", dist), ("1", found), ("1", "check must be 0 or 1"),
            ("1", "speckle max_size must be >= 0")]
    assert [tuple(g) for g in got] == want


# ---- the rule on the cross-view scene ----------------------------------------------
@pytest.fixture(scope="module")
def scene_maps():
    """The CPU expectation of the checked and speckle-filtered maps (CHECK, 20 / 1)."""
    checked = cs.checked(**cs.CHECK)[0]
    return se.filter_speckles(checked, cs.INVALID, 20, 1)[0]


def fill_quality(before, after):
    """(holes, filled, right, wrong) over the interior of all nine views: right =
    filled and |d - truth| <= 1."""
    t = cs.views_and_truth()[1][cs.INTERIOR]
    b, a = before[cs.INTERIOR], after[cs.INTERIOR]
    hole = ~fe.valid(b, cs.INVALID)
    filled = hole & fe.valid(a, cs.INVALID)
    wrong = filled & (np.abs(a.astype(np.int64) - t) > 1)
    return int(hole.sum()), int(filled.sum()), int((filled & ~wrong).sum()), int(wrong.sum())


# mode: (holes, filled, right, wrong); the frame before the fill has 454 wrong and
# 65,532 correct pixels (tests/test_speckle_cpu.py) and 1,406 holes
QUALITY = {fe.MIN: (1406, 1406, 1082, 324), fe.SECOND: (1406, 1406, 1093, 313),
           fe.MEDIAN: (1406, 1406, 1137, 269)}


@pytest.mark.parametrize("mode", fe.MODES)
def test_scene_quality_table(scene_maps, mode):
    """DESIGN.md §2.5d's table: max_dist 16, min_found 3.  The counts are the
    rule's, pinned as fill_expect produces them."""
    out, _, _, filled = fe.fill_holes(scene_maps, cs.INVALID, 16, 3, mode)
    q = fill_quality(scene_maps, out)
    print("mode %d: holes %d filled %d right %d wrong %d" % ((mode,) + q))
    assert q == QUALITY[mode]
    assert q[1] == int(filled[cs.INTERIOR].sum())
    # what was valid keeps its value, so the frame's earlier counts stand
    ok = fe.valid(scene_maps, cs.INVALID)
    assert np.array_equal(out[ok], scene_maps[ok])
