"""The speckle filter without a GPU: host programs, each with
its own main, built under AddressSanitizer and UBSan, and the rule's effect on
the cross-view scene.

1. csrc/speckle_math.h -- linked, removed, the clamp -- over a dumped case set
   against speckle_expect.
2. csrc/speckle_uf.h run sequentially: the program emulates the four passes
   (label per tile, merge over the border links in random order, count, apply)
   with a tile shape from the command line, on plain memory and under a stale
   policy whose load returns, at random, any value the word has held since the
   last launch boundary.  Outputs and sizes must equal speckle_expect; the
   program asserts its own step bound.
3. The rules sva_array_depth_filtered adds to check_array_args, alone and in pairs.
4. speckle_expect itself against a transitive closure on frames up to 4x4, and
   the quality table of DESIGN.md §2.5c on tests/cross_scene.py.
Nothing is loaded into Python under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

import cross_expect as ce
import cross_scene as cs
import speckle_expect as se

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereovisionarray_amd", "csrc")
INC = os.path.join(ROOT, "include")
OK, INVALID, UNSUPPORTED = 0, 1, 2


def build(d, name, text):
    src = d / (name + ".cpp")
    src.write_text(text)
    exe = d / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-g", "-I", CSRC, "-I", INC, str(src), "-o",
                    str(exe)], check=True)
    return str(exe)


# ---- the expectation itself --------------------------------------------------------
def test_expectation_equals_transitive_closure():
    rng = np.random.default_rng(11)
    seen = set()
    for _ in range(600):
        H, W = (int(v) for v in rng.integers(1, 5, 2))
        inv = int(rng.choice([0xFFFF, 3]))
        d = rng.integers(0, 6, (H, W)).astype(np.uint16)
        d[rng.random((H, W)) < 0.1] = inv
        md = int(rng.choice([0, 1, 2, 65535]))
        size = se.comp_size_map(d, inv, md)
        assert np.array_equal(size, se.closure_size(d, inv, md)), (d, inv, md)
        assert ((size == 0) == ~se.valid(d, inv)).all()
        seen |= set(size.ravel().tolist())
    assert {0, 1, 2, 3, 16} <= seen
    for f in (se.snake, se.spiral, se.checkerboard, se.solid, se.u_shape):
        for W, H in ((4, 4), (3, 4), (1, 4), (4, 1)):
            d = f(W, H)
            for md in (0, 2):
                assert np.array_equal(se.comp_size_map(d, 0xFFFF, md), se.closure_size(d, 0xFFFF, md))


# ---- speckle_math.h ----------------------------------------------------------------
MATH_PROGRAM = r"""
#include <cstdio>
#include "speckle_math.h"
using namespace sva;
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    long long s, t, invalid, md, size, ms;
    while (std::fscanf(f, "%lld %lld %lld %lld %lld %lld", &s, &t, &invalid, &md, &size, &ms) == 6) {
        const int c = sp::clamp_diff((int)md);
        std::printf("%d %d %d %d\n", (int)sp::linked((unsigned)s, (unsigned)t, (unsigned)invalid, c),
                    (int)sp::removed((uint32_t)size, (int)ms), c,
                    (int)(sp::thresholds_error((int)ms, (int)md) == nullptr));
    }
    std::fclose(f);
    return 0;
}
"""


def math_cases():
    """Rows (s, t, invalid, max_diff, size, max_size)."""
    rng = np.random.default_rng(78)
    big = 2 ** 31 - 1
    rows = []
    for _ in range(4000):
        inv = int(rng.choice([0xFFFF, 0, 77, 40000]))
        s = int(rng.choice([rng.integers(0, 41), rng.integers(0, 65536), inv, 0]))
        md = int(rng.choice([0, 1, 3, 65534, 65535, 65536, big]))
        t = int(rng.choice([rng.integers(0, 41), rng.integers(0, 65536), inv, 0, s,
                            max(s - min(md, 65535), 0), min(s + min(md, 65535), 65535)]))
        size = int(rng.choice([0, 1, 2, 20, 21, rng.integers(0, 2 ** 31)]))
        ms = int(rng.choice([0, 1, 20, size, max(size - 1, 0), min(size + 1, big), big]))
        rows.append((s, t, inv, md, size, ms))
    # the borders |s - t| = max_diff and max_diff + 1, both ways round
    for s in (1, 20, 30000, 65535, 65534):
        for md in (0, 1, 3, 65533, 65534, 65535):
            for t in {s - md, s - md - 1, s + md, s + md + 1}:
                if 0 <= t <= 65535:
                    for inv in (0xFFFF, 77):
                        rows.append((s, t, inv, md, 5, 5))
    # s or t equal to invalid or 0
    for inv in (0xFFFF, 77, 0):
        for a in (inv, 0, 9):
            for b in (inv, 0, 9):
                rows.append((a, b, inv, 65535, 1, 0))
    return np.array(rows, dtype=np.int64)


def test_math_header_equals_speckle_expect(tmp_path):
    exe = build(tmp_path, "specklemath", MATH_PROGRAM)
    rows = math_cases()
    path = tmp_path / "cases.txt"
    np.savetxt(path, rows, fmt="%d")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    got = np.array([[int(v) for v in line.split()] for line in run.stdout.splitlines()])
    assert got.shape == (len(rows), 4)
    linked = np.array([bool(se.links(np.array([[s, t]]), inv, md)[0][0, 0])
                       for s, t, inv, md, _, _ in rows])
    assert linked.any() and (~linked).any()
    assert np.array_equal(got[:, 0], linked.astype(np.int64))
    gone = np.array([bool(se.apply(np.array([[9]], np.uint16), np.array([[size]]), 0xFFFF, ms)[2][0, 0])
                     for _, _, _, _, size, ms in rows])
    assert gone.any() and (~gone).any()
    assert np.array_equal(got[:, 1], gone.astype(np.int64))
    assert np.array_equal(got[:, 2], np.minimum(rows[:, 3], 65535))
    assert (got[:, 3] == 1).all()


# ---- speckle_uf.h ------------------------------------------------------------------
UF_PROGRAM = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "speckle_math.h"
#include "speckle_uf.h"
using namespace sva;

// Plain memory, or stale: load returns any value the word has held since the
// last boundary (the launch boundary makes earlier writes visible).  steps
// counts the loop iterations of find and unite: a load that moves find on, and
// an exchange.
struct Mem {
    std::vector<uint32_t> l;
    std::vector<std::vector<uint32_t>> held;
    bool stale = false;
    std::mt19937* rng = nullptr;
    unsigned long long steps = 0;
    void boundary() { for (auto& h : held) h.clear(); }
    uint32_t load(uint32_t i) {
        uint32_t v = l.at(i);
        if (stale && !held.at(i).empty()) {
            const size_t k = (*rng)() % (held[i].size() + 1);
            if (k < held[i].size()) v = held[i][k];
        }
        if (v < i) steps++;
        return v;
    }
    uint32_t min_exchange(uint32_t i, uint32_t v) {
        steps++;
        const uint32_t old = l.at(i);
        if (v < old) {
            if (stale) held.at(i).push_back(old);
            l[i] = v;
        }
        return old;
    }
};

int main(int argc, char** argv) {
    if (argc != 10) return 2;
    const int W = std::atoi(argv[1]), H = std::atoi(argv[2]), TW = std::atoi(argv[3]),
              TH = std::atoi(argv[4]);
    const unsigned invalid = (unsigned)std::atoi(argv[5]);
    const int md = sp::clamp_diff(std::atoi(argv[6])), ms = std::atoi(argv[7]);
    const bool stale = std::atoi(argv[8]) != 0;
    std::FILE* f = std::fopen(argv[9], "r");
    if (!f) return 2;
    const uint32_t np = (uint32_t)W * H;
    std::vector<unsigned> d(np);
    for (auto& v : d)
        if (std::fscanf(f, "%u", &v) != 1) return 2;
    std::fclose(f);
    std::mt19937 rng(12345u + W * 7 + TW);
    const int tx = (W + TW - 1) / TW, ty = (H + TH - 1) / TH, TP = TW * TH;
    Mem g;
    g.l.assign(np, sp::kNoLabel);
    g.held.resize(np);
    g.stale = stale;
    g.rng = &rng;
    std::vector<uint32_t> count(np, 0);

    // ---- label: per tile, on tile-local indices
    for (int t = 0; t < tx * ty; t++) {
        const int x0 = (t % tx) * TW, y0 = (t / tx) * TH;
        Mem m;
        m.l.resize(TP);
        m.held.resize(TP);
        m.stale = stale;
        m.rng = &rng;
        std::vector<unsigned> sd(TP, 0);
        for (int i = 0; i < TP; i++) {
            const int x = x0 + i % TW, y = y0 + i / TW;
            if (x < W && y < H) sd[i] = d[(size_t)y * W + x];
            m.l[i] = (uint32_t)i;
        }
        std::vector<int> order(TP);
        for (int i = 0; i < TP; i++) order[i] = i;
        std::shuffle(order.begin(), order.end(), rng);
        unsigned long long links = 0;
        for (int i : order) {
            if (i % TW + 1 < TW && sp::linked(sd[i], sd[i + 1], invalid, md)) {
                uf::unite(m, (uint32_t)i, (uint32_t)i + 1);
                links++;
            }
            if (i / TW + 1 < TH && sp::linked(sd[i], sd[i + TW], invalid, md)) {
                uf::unite(m, (uint32_t)i, (uint32_t)i + TW);
                links++;
            }
        }
        if (m.steps > (unsigned long long)TP * links) {
            std::fprintf(stderr, "label steps %llu > %d * %llu\n", m.steps, TP, links);
            return 3;
        }
        m.boundary();   // the workgroup barrier
        std::vector<uint32_t> root(TP, sp::kNoLabel), sc(TP, 0);
        for (int i = 0; i < TP; i++)
            if (cc::valid(sd[i], invalid)) {
                root[i] = uf::find(m, (uint32_t)i);
                sc.at(root[i])++;
            }
        for (int i = 0; i < TP; i++) {
            const int x = x0 + i % TW, y = y0 + i / TW;
            if (x >= W || y >= H) continue;
            const uint32_t r = root[i];
            const size_t at = (size_t)y * W + x;
            g.l[at] = r == sp::kNoLabel ? sp::kNoLabel
                                        : (uint32_t)((y0 + r / TW) * W + x0 + r % TW);
            if (g.l[at] != sp::kNoLabel && g.l[at] > at) return 4;   // label[i] <= i
            count[at] = r == (uint32_t)i ? sc[i] : 0u;
        }
    }

    // ---- merge: the border links, in the kernel's enumeration, shuffled
    std::vector<std::pair<uint32_t, uint32_t>> edges;
    for (int y = 0; y < H; y++)
        for (int k = 1; k < tx; k++) edges.push_back({(uint32_t)(y * W + k * TW - 1), (uint32_t)(y * W + k * TW)});
    for (int k = 1; k < ty; k++)
        for (int x = 0; x < W; x++) edges.push_back({(uint32_t)((k * TH - 1) * W + x), (uint32_t)(k * TH * W + x)});
    std::shuffle(edges.begin(), edges.end(), rng);
    g.steps = 0;
    const std::vector<uint32_t> before = g.l;
    for (auto& e : edges)
        if (sp::linked(d[e.first], d[e.second], invalid, md)) uf::unite(g, e.first, e.second);
    if (g.steps > (unsigned long long)np * edges.size()) {
        std::fprintf(stderr, "merge steps %llu > %u * %zu\n", g.steps, np, edges.size());
        return 3;
    }
    for (uint32_t p = 0; p < np; p++)   // labels only decrease, label[i] <= i
        if (g.l[p] > before[p] || (g.l[p] != sp::kNoLabel && g.l[p] > p)) return 4;
    g.boundary();

    // ---- count: tile-local roots, in random order, with path compression
    std::vector<uint32_t> order(np);
    for (uint32_t p = 0; p < np; p++) order[p] = p;
    std::shuffle(order.begin(), order.end(), rng);
    std::vector<uint32_t> local = count;
    for (uint32_t p : order) {
        if (local[p] == 0) continue;
        const uint32_t r = uf::find(g, p);
        if (r == p) continue;
        count.at(r) += local[p];
        g.min_exchange(p, r);
    }
    g.boundary();

    // ---- apply
    for (uint32_t p = 0; p < np; p++) {
        uint32_t size = 0;
        if (cc::valid(d[p], invalid)) size = count.at(uf::find(g, p));
        std::printf("%u %u\n", sp::removed(size, ms) ? invalid : d[p], size);
    }
    return 0;
}
"""

TILES = [(1, 1), (3, 2), (64, 16)]
UF_FRAMES = {
    "random": lambda W, H: se.random_map(W, H, 5),
    "random_levels2": lambda W, H: se.random_map(W, H, 6, levels=2),
    "snake": se.snake,
    "spiral": se.spiral,
    "checkerboard": se.checkerboard,
    "solid": se.solid,
    "ring": se.u_shape,
}


@pytest.fixture(scope="module")
def uf_exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("speckleuf"), "speckleuf", UF_PROGRAM)


@pytest.mark.parametrize("stale", [0, 1], ids=["plain", "stale"])
@pytest.mark.parametrize("tile", TILES, ids=lambda t: "%dx%d" % t)
@pytest.mark.parametrize("frame", sorted(UF_FRAMES))
def test_union_find_passes_equal_expectation(uf_exe, tmp_path, frame, tile, stale):
    """Frames a little larger than two tiles each way (and 13x9 for the 1x1 and
    3x2 tiles), so every shape crosses borders in both directions."""
    tw, th = tile
    for W, H in ((13, 9), (2 * tw + 3, 2 * th + 1)) if tw * th < 64 else ((2 * tw + 3, 2 * th + 1),
                                                                          (tw + 1, 3 * th + 1)):
        d = UF_FRAMES[frame](W, H)
        path = tmp_path / "map.txt"
        np.savetxt(path, d.astype(np.int64), fmt="%d")
        for md, ms in ((0, 3), (1, 20)):
            run = subprocess.run([uf_exe, str(W), str(H), str(tw), str(th), str(0xFFFF), str(md),
                                  str(ms), str(stale), str(path)], capture_output=True, text=True)
            assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr)
            got = np.array([[int(v) for v in line.split()] for line in run.stdout.splitlines()])
            eo, _, size = se.filter_speckles(d, 0xFFFF, ms, md)
            assert np.array_equal(got[:, 1].reshape(H, W), size), (W, H, md)
            assert np.array_equal(got[:, 0].reshape(H, W), eo), (W, H, md, ms)


# ---- check_array_args ----------------------------------------------------------------
ARGS_PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "array_args.h"
using namespace sva;

// Views 0..2 at grid (0,0), (1,0), (0,1): view_step = -grid.  Group g = reference
// g against the other two.  kind 0: GROUPS, check 1; 1: GROUPS, check 0; 2: PAIRS,
// check 0 (MIN_COST fusion with a winner map, per-pair lr_check).
struct Frame {
    std::vector<uint8_t> pixel = std::vector<uint8_t>(1);
    std::vector<const uint8_t*> images;
    std::vector<sva_array_pair> pairs;
    std::vector<int32_t> gs, vs = {0, 0, -1, 0, 0, -1};
    std::vector<double> depth = std::vector<double>(1);
    std::vector<float> subpix = std::vector<float>(1);
    std::vector<uint8_t> plane = std::vector<uint8_t>(1);
    std::vector<uint32_t> size = std::vector<uint32_t>(1);
    ArrayArgs a;

    // what sva_array_depth_filtered does with its `check`
    void set_check(int check) {
        a.check = check;
        a.cross = check == 1;
        a.view_step = a.cross ? vs.data() : nullptr;
        a.max_diff = a.cross ? 1 : 0;
        a.min_agree = a.cross ? 2 : 0;
        a.max_conflict = 0;
    }
    explicit Frame(int kind) {
        gs.push_back(0);
        for (int g = 0; g < 3; g++) {
            for (int o = 0; o < 3; o++) {
                if (o == g) continue;
                sva_array_pair q;
                std::memset(&q, 0, sizeof q);
                q.ref = g;
                q.other = o;
                q.params.D = 64;
                q.params.P1 = 10;
                q.params.P2 = 120;
                q.params.invalid = 0xffff;
                const int ex = vs[2 * o] - vs[2 * g], ey = vs[2 * o + 1] - vs[2 * g + 1];
                q.params.dir = ex;
                q.params.dir_y = ey;
                q.params.lr_check = kind == 2;
                q.baseline = 0.05;
                pairs.push_back(q);
            }
            gs.push_back((int)pairs.size());
        }
        images.assign(3, pixel.data());
        a.images = images.data();
        a.n_images = 3;
        a.W = a.H = 20;
        a.pitch = 20;
        a.pairs = pairs.data();
        a.n_pairs = (int)pairs.size();
        a.group_start = gs.data();
        a.n_groups = 3;
        a.f = 0.05;
        a.pixel_size = 1e-5;
        a.depth = depth.data();
        a.route = kind == 2 ? ArrayRoute::Pairs : ArrayRoute::Groups;
        a.conf = true;
        a.mode = kind == 2 ? SVA_FUSE_MIN_COST : SVA_FUSE_MEDIAN;
        a.winner = kind == 2 ? plane.data() : nullptr;
        a.speckle = true;
        a.speckle_max_size = 20;
        a.speckle_max_diff = 1;
        a.comp_size = size.data();
        set_check(kind == 0);
    }
};

struct Case {
    const char* name;
    void (*mutate)(Frame&);
};
const Case kCases[] = {
    {"valid", [](Frame&) {}},
    {"check_2", [](Frame& f) { f.set_check(2); }},
    {"check_negative", [](Frame& f) { f.set_check(-1); }},
    {"check_flipped", [](Frame& f) { f.set_check(f.a.check ? 0 : 1); }},
    {"agree", [](Frame& f) { f.a.agree = f.plane.data(); }},
    {"conflict", [](Frame& f) { f.a.conflict = f.plane.data(); }},
    {"subpix_without_sub", [](Frame& f) { f.a.subpix = f.subpix.data(); }},
    {"subpix_with_sub", [](Frame& f) { f.a.sub = true; f.a.subpix = f.subpix.data(); }},
    {"max_size_negative", [](Frame& f) { f.a.speckle_max_size = -1; }},
    {"max_size_zero", [](Frame& f) { f.a.speckle_max_size = 0; }},
    {"max_size_largest", [](Frame& f) { f.a.speckle_max_size = 0x7fffffff; }},
    {"max_diff_negative", [](Frame& f) { f.a.speckle_max_diff = -1; }},
    {"max_diff_largest", [](Frame& f) { f.a.speckle_max_diff = 0x7fffffff; }},
    {"no_comp_size", [](Frame& f) { f.a.comp_size = nullptr; }},
    {"lr_check", [](Frame& f) { f.pairs[0].params.lr_check = 1; }},
    // two rules at once: the first in the documented order
    {"bad_pair_and_check_2", [](Frame& f) { f.pairs[0].ref = -1; f.set_check(2); }},
    {"check_2_and_agree", [](Frame& f) { f.set_check(2); f.a.agree = f.plane.data(); }},
    {"check_2_and_max_size", [](Frame& f) { f.set_check(2); f.a.speckle_max_size = -1; }},
    {"agree_and_subpix", [](Frame& f) { f.a.agree = f.plane.data(); f.a.subpix = f.subpix.data(); }},
    {"agree_and_max_size", [](Frame& f) { f.a.agree = f.plane.data(); f.a.speckle_max_size = -1; }},
    {"subpix_and_max_size", [](Frame& f) { f.a.subpix = f.subpix.data(); f.a.speckle_max_size = -1; }},
    {"max_size_and_max_diff", [](Frame& f) { f.a.speckle_max_size = -1; f.a.speckle_max_diff = -1; }},
    {"min_agree_and_max_size", [](Frame& f) { f.a.min_agree = 32; f.a.speckle_max_size = -1; }},
    // the flag off: the filter's fields are not looked at
    {"not_filtered", [](Frame& f) { f.a.speckle = false; f.a.check = 7; f.a.speckle_max_size = -1; }},
};

int main() {
    for (int kind = 0; kind < 3; kind++)
        for (const Case& c : kCases) {
            Frame f(kind);
            c.mutate(f);
            std::string msg;
            std::vector<int32_t> ratio;
            const int st = check_array_args(f.a, msg, ratio);
            std::printf("%s|%d|%d|%s\n", c.name, kind, st, msg.c_str());
        }
    return 0;
}
"""

CHECK_MSG = "check must be 0 or 1"
COUNTS_MSG = "agree and conflict need check = 1"
SUB_MSG = "subpix needs sub = 1"
SIZE_MSG = "speckle max_size must be >= 0"
DIFF_MSG = "speckle max_diff must be >= 0"
NEEDS_GROUPS = ("the cross-view check needs a group route: the pair route's maps share one "
                "reference camera")
NO_LR = "the multi-baseline route has no L/R check"
# (case, then (status, message) for GROUPS check 1, GROUPS check 0, PAIRS check 0)
RULES = [
    ("valid", (OK, ""), (OK, ""), (OK, "")),
    ("check_2", (INVALID, CHECK_MSG), (INVALID, CHECK_MSG), (INVALID, CHECK_MSG)),
    ("check_negative", (INVALID, CHECK_MSG), (INVALID, CHECK_MSG), (INVALID, CHECK_MSG)),
    ("check_flipped", (OK, ""), (OK, ""), (UNSUPPORTED, NEEDS_GROUPS)),
    ("agree", (OK, ""), (INVALID, COUNTS_MSG), (INVALID, COUNTS_MSG)),
    ("conflict", (OK, ""), (INVALID, COUNTS_MSG), (INVALID, COUNTS_MSG)),
    ("subpix_without_sub", (INVALID, SUB_MSG), (INVALID, SUB_MSG), (INVALID, SUB_MSG)),
    ("subpix_with_sub", (OK, ""), (OK, ""), (OK, "")),
    ("max_size_negative", (INVALID, SIZE_MSG), (INVALID, SIZE_MSG), (INVALID, SIZE_MSG)),
    ("max_size_zero", (OK, ""), (OK, ""), (OK, "")),
    ("max_size_largest", (OK, ""), (OK, ""), (OK, "")),
    ("max_diff_negative", (INVALID, DIFF_MSG), (INVALID, DIFF_MSG), (INVALID, DIFF_MSG)),
    ("max_diff_largest", (OK, ""), (OK, ""), (OK, "")),
    ("no_comp_size", (OK, ""), (OK, ""), (OK, "")),
    ("lr_check", (UNSUPPORTED, NO_LR), (UNSUPPORTED, NO_LR), (OK, "")),
    ("bad_pair_and_check_2", (INVALID, "bad pair 0"), (INVALID, "bad pair 0"), (INVALID, "bad pair 0")),
    ("check_2_and_agree", (INVALID, CHECK_MSG), (INVALID, CHECK_MSG), (INVALID, CHECK_MSG)),
    ("check_2_and_max_size", (INVALID, CHECK_MSG), (INVALID, CHECK_MSG), (INVALID, CHECK_MSG)),
    ("agree_and_subpix", (INVALID, SUB_MSG), (INVALID, COUNTS_MSG), (INVALID, COUNTS_MSG)),
    ("agree_and_max_size", (INVALID, SIZE_MSG), (INVALID, COUNTS_MSG), (INVALID, COUNTS_MSG)),
    ("subpix_and_max_size", (INVALID, SUB_MSG), (INVALID, SUB_MSG), (INVALID, SUB_MSG)),
    ("max_size_and_max_diff", (INVALID, SIZE_MSG), (INVALID, SIZE_MSG), (INVALID, SIZE_MSG)),
    ("min_agree_and_max_size", (INVALID, "min_agree must be 0..31"), (INVALID, SIZE_MSG),
     (INVALID, SIZE_MSG)),
    ("not_filtered", (OK, ""), (OK, ""), (OK, "")),
]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    exe = build(tmp_path_factory.mktemp("speckleargs"), "speckleargs", ARGS_PROGRAM)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    out = {}
    for line in run.stdout.splitlines():
        name, kind, status, msg = line.split("|", 3)
        out[(name, int(kind))] = (int(status), msg)
    return out


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["groups_checked", "groups", "pairs"])
@pytest.mark.parametrize("rule", RULES, ids=lambda r: r[0])
def test_rule(answers, rule, kind):
    assert answers[(rule[0], kind)] == rule[1 + kind]


# ---- the scene ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    return cs.matched()[0], cs.checked(**cs.CHECK)[0]


def test_scene_quality_table(scene):
    """DESIGN.md §2.5c's table: (wrong, correct) over the interior of the nine
    maps, max_size 20, max_diff 1."""
    matched, checked = scene
    assert cs.quality(matched) == (1444, 65948) and cs.quality(checked) == (552, 65591)
    f_matched = se.filter_speckles(matched, cs.INVALID, 20, 1)[0]
    f_checked = se.filter_speckles(checked, cs.INVALID, 20, 1)[0]
    assert cs.quality(f_matched) == (1193, 65893)
    assert cs.quality(f_checked) == (454, 65532)
    then_checked = ce.cross_check(f_matched, cs.VIEW_STEP, cs.INVALID, **cs.CHECK)[0]
    assert cs.quality(then_checked) == (474, 65545)


@pytest.mark.parametrize("max_size,max_diff,expected", [
    (8, 1, (454, 65532)), (400, 1, (454, 65532)), (8, 0, (285, 63729)), (400, 0, (260, 63305))])
def test_scene_other_thresholds(scene, max_size, max_diff, expected):
    """After the check, max_size from 8 to 400 changes nothing at max_diff 1;
    max_diff 0 removes more and costs 3 % of the correct pixels."""
    assert cs.quality(se.filter_speckles(scene[1], cs.INVALID, max_size, max_diff)[0]) == expected
