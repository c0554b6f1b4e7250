"""The cross-view consistency check without a GPU: two host
programs, each with its own main, built under AddressSanitizer and UBSan.

The first runs csrc/cross_check_math.h -- the inside test and the four-way
classification the kernel compiles -- over a dumped case set and prints what it
answers; cross_expect must say the same.  The second breaks every rule that
sva_array_depth_checked adds to check_array_args (csrc/array_args.h), one at a
time and two at a time, and prints status and message.  Nothing is loaded into
Python under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

import cross_expect as ce

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereovisionarray_amd", "csrc")
INC = os.path.join(ROOT, "include")
OK, INVALID, UNSUPPORTED = 0, 1, 2


def build(d, name, text):
    src = d / (name + ".cpp")
    src.write_text(text)
    exe = d / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-g", "-I", CSRC, "-I", INC, str(src), "-o",
                    str(exe)], check=True)
    return str(exe)


# ---- cross_check_math.h ----------------------------------------------------------
MATH_PROGRAM = r"""
#include <cstdio>
#include "cross_check_math.h"
using namespace sva;
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    long long px, py, s, ex, ey, W, H, t, invalid, md;
    while (std::fscanf(f, "%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", &px, &py, &s, &ex,
                       &ey, &W, &H, &t, &invalid, &md) == 10) {
        int qx = -1, qy = -1;
        const bool in = cc::inside((int)px, (int)py, (int)s, (int)ex, (int)ey, (int)W, (int)H, &qx, &qy);
        const int cls = cc::classify((int)s, (unsigned)t, (unsigned)invalid, (int)md);
        std::printf("%d %d %d %d %d %d\n", (int)in, in ? qx : -1, in ? qy : -1, cls,
                    (int)cc::valid((unsigned)s, (unsigned)invalid),
                    (int)cc::keep((int)(t % 32), (int)(s % 32), (int)(md % 32), (int)(px % 32)));
    }
    std::fclose(f);
    return 0;
}
"""


def math_cases():
    """Rows (px, py, s, ex, ey, W, H, t, invalid, max_diff)."""
    rng = np.random.default_rng(77)
    rows = []
    for _ in range(4000):
        W, H = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        inv = int(rng.choice([0xFFFF, 0, 77, 40000]))
        s = int(rng.choice([rng.integers(0, 41), rng.integers(0, 65536), inv]))
        t = int(rng.choice([rng.integers(0, 41), rng.integers(0, 65536), inv, s, max(s - 1, 0),
                            min(s + 1, 65535)]))
        rows.append((int(rng.integers(0, W)), int(rng.integers(0, H)), s,
                     int(rng.integers(-510, 511)), int(rng.integers(-510, 511)), W, H, t, inv,
                     int(rng.choice([0, 1, 3, 65535]))))
    # the largest products: s = 65535 along e = +-510, inside and outside a huge row / column
    big = 2 ** 31 - 1
    far = 65535 * 510
    for e in (510, -510):
        for p in (0, far, big - 1 - far, big - 1, far - 1, big - far):
            rows.append((p, 0, 65535, e, 0, big, 1, 9, 0xFFFF, 1))
            rows.append((0, p, 65535, 0, e, 1, big, 9, 0xFFFF, 1))
            rows.append((p, 0, 65535, e, e, big, 1, 9, 0xFFFF, 1))
    # q exactly on each of the four edges, and one pixel outside each
    W, H, s = 70, 37, 5
    for qx, qy in ((0, 11), (W - 1, 11), (13, 0), (13, H - 1), (-1, 11), (W, 11), (13, -1),
                   (13, H), (0, 0), (W - 1, H - 1), (-1, -1), (W, H)):
        for ex, ey in ((1, 0), (-1, 0), (0, 1), (0, -1), (2, -3), (-3, 2)):
            px, py = qx - s * ex, qy - s * ey
            if 0 <= px < W and 0 <= py < H:
                rows.append((px, py, s, ex, ey, W, H, 5, 0xFFFF, 0))
    # the classification's borders
    for s in (1, 20, 65535):
        for md in (0, 1, 3, 65535):
            for t in {0, 0xFFFF, s, max(s - md, 0), max(s - md - 1, 0), min(s + md, 65535),
                      min(s + md + 1, 65535)}:
                rows.append((0, 0, s, 0, 0, 1, 1, t, 0xFFFF, md))
    return np.array(rows, dtype=np.int64)


def test_math_header_equals_cross_expect(tmp_path):
    exe = build(tmp_path, "crossmath", MATH_PROGRAM)
    rows = math_cases()
    path = tmp_path / "cases.txt"
    np.savetxt(path, rows, fmt="%d")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    got = np.array([[int(v) for v in line.split()] for line in run.stdout.splitlines()])
    assert got.shape == (len(rows), 6)
    px, py, s, ex, ey, W, H, t, inv, md = rows.T
    qx, qy, ins = ce.target(px, py, s, ex, ey, W, H)
    assert ins.any() and (~ins).any()
    assert np.array_equal(got[:, 0], ins.astype(np.int64))
    assert np.array_equal(got[:, 1], np.where(ins, qx, -1))
    assert np.array_equal(got[:, 2], np.where(ins, qy, -1))
    cls = np.array([int(ce.classes(a, b, c, d)) for a, b, c, d in zip(s, t, inv, md)])
    assert set(cls) == {ce.NONE, ce.AGREE, ce.CONFLICT, ce.OCCLUDED}
    assert np.array_equal(got[:, 3], cls)
    assert np.array_equal(got[:, 4], ce.valid(s, inv).astype(np.int64))
    assert np.array_equal(got[:, 5], ((t % 32 >= md % 32) & (s % 32 <= px % 32)).astype(np.int64))
    # the edge rows were there: a q on every edge and one pixel past it
    edge = (W == 70) & (H == 37)
    assert {(0, 11), (69, 11), (13, 0), (13, 36)} <= set(zip(qx[edge & ins], qy[edge & ins]))
    assert {(-1, 11), (70, 11), (13, -1), (13, 37)} <= set(zip(qx[edge & ~ins], qy[edge & ~ins]))


# ---- check_array_args -----------------------------------------------------------
ARGS_PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "array_args.h"
using namespace sva;

// Views 0..3 at grid (0,0), (1,0), (0,1), (2,0): view_step = -grid.  Group g =
// reference g against the other two of views 0..2; on the mixed route group 0
// also matches view 3 at twice the unit baseline.  Every array is a heap array
// of exactly its length.
struct Frame {
    std::vector<uint8_t> pixel = std::vector<uint8_t>(1);
    std::vector<const uint8_t*> images;
    std::vector<sva_array_pair> pairs;
    std::vector<int32_t> gs, vs;
    std::vector<double> unit, depth = std::vector<double>(1);
    std::vector<float> subpix = std::vector<float>(1);
    ArrayArgs a;

    void pair(int ref, int other, double baseline) {
        sva_array_pair q;
        std::memset(&q, 0, sizeof q);
        q.ref = ref;
        q.other = other;
        q.params.D = 64;
        q.params.P1 = 10;
        q.params.P2 = 120;
        q.params.invalid = 0xffff;
        int ex = vs[2 * other] - vs[2 * ref], ey = vs[2 * other + 1] - vs[2 * ref + 1];
        const int m = std::max(std::abs(ex), std::abs(ey));
        q.params.dir = ex / m;          // the frames here have steps along one axis or diagonal
        q.params.dir_y = ey / m;
        q.baseline = baseline;
        pairs.push_back(q);
    }
    void finish(bool mixed, int sub) {
        images.assign(vs.size() / 2, pixel.data());
        unit.assign(gs.size() - 1, 0.05);
        a.images = images.data();
        a.n_images = (int)images.size();
        a.W = a.H = 20;
        a.pitch = 20;
        a.pairs = pairs.data();
        a.n_pairs = (int)pairs.size();
        a.group_start = gs.data();
        a.n_groups = (int)gs.size() - 1;
        a.f = 0.05;
        a.pixel_size = 1e-5;
        a.depth = depth.data();
        a.route = mixed ? ArrayRoute::GroupsMixed : ArrayRoute::Groups;
        a.conf = true;
        a.sub = sub != 0;
        a.unit_baseline = mixed ? unit.data() : nullptr;
        a.cross = true;
        a.view_step = vs.data();
        a.max_diff = 1;
        a.min_agree = 2;
        a.max_conflict = 0;
    }
    // the three-camera frame
    Frame(bool mixed, int sub) {
        vs = {0, 0, -1, 0, 0, -1, -2, 0};
        gs.push_back(0);
        for (int g = 0; g < 3; g++) {
            for (int o = 0; o < 3; o++)
                if (o != g) pair(g, o, 0.05);
            if (mixed && g == 0) pair(0, 3, 0.1);
            gs.push_back((int)pairs.size());
        }
        finish(mixed, sub);
    }
    // n cameras on a line from x0 leftwards, group g = camera g against its neighbour
    Frame(int n, int x0) {
        for (int v = 0; v < n; v++) {
            vs.push_back(x0 - v);
            vs.push_back(0);
        }
        gs.push_back(0);
        for (int g = 0; g < n; g++) {
            pair(g, g + 1 < n ? g + 1 : g - 1, 0.05);
            gs.push_back((int)pairs.size());
        }
        finish(false, 0);
    }
};

void report(const char* name, int kind, const ArrayArgs& a) {
    std::string msg;
    std::vector<int32_t> ratio;
    const int st = check_array_args(a, msg, ratio);
    std::printf("%s|%d|%d|%s\n", name, kind, st, msg.c_str());
}

struct Case {
    const char* name;
    void (*mutate)(Frame&);
};
#define P(j) f.pairs[j]
const Case kCases[] = {
    {"valid", [](Frame&) {}},
    {"pair_route", [](Frame& f) { f.a.route = ArrayRoute::Pairs; f.a.unit_baseline = nullptr; }},
    {"subpix_without_sub", [](Frame& f) { f.a.subpix = f.a.sub ? nullptr : f.subpix.data(); }},
    {"null_view_step", [](Frame& f) { f.a.view_step = nullptr; }},
    {"same_ref", [](Frame& f) {
         for (int j = f.gs[1]; j < f.gs[2]; j++) { P(j).ref = 0; P(j).other = 1 + (j - f.gs[1]); }
     }},
    {"invalid_differs",
     [](Frame& f) { for (int j = f.gs[1]; j < f.gs[2]; j++) P(j).params.invalid = 0; }},
    {"scale_differs", [](Frame& f) {
         if (f.a.unit_baseline) f.unit[1] = 0.1;
         else for (int j = f.gs[1]; j < f.gs[2]; j++) P(j).baseline = 0.1;
     }},
    {"geometry", [](Frame& f) { f.vs[5] = -2; }},
    {"geometry_sign", [](Frame& f) { P(0).params.dir = -P(0).params.dir; }},
    {"max_diff_negative", [](Frame& f) { f.a.max_diff = -1; }},
    {"max_diff_huge", [](Frame& f) { f.a.max_diff = 0x7fffffff; }},
    {"min_agree_32", [](Frame& f) { f.a.min_agree = 32; }},
    {"min_agree_negative", [](Frame& f) { f.a.min_agree = -1; }},
    {"min_agree_31", [](Frame& f) { f.a.min_agree = 31; }},
    {"max_conflict_32", [](Frame& f) { f.a.max_conflict = 32; }},
    {"max_conflict_negative", [](Frame& f) { f.a.max_conflict = -1; }},
    {"max_conflict_31", [](Frame& f) { f.a.max_conflict = 31; }},
    // two rules at once: the first in the documented order
    {"lr_check_and_null_view_step",
     [](Frame& f) { P(0).params.lr_check = 1; f.a.view_step = nullptr; }},
    {"bad_pair_and_pair_route", [](Frame& f) {
         P(0).ref = -1;
         f.a.route = ArrayRoute::Pairs;
         f.a.unit_baseline = nullptr;
     }},
    {"pair_route_and_null_view_step", [](Frame& f) {
         f.a.route = ArrayRoute::Pairs;
         f.a.unit_baseline = nullptr;
         f.a.view_step = nullptr;
     }},
    {"null_view_step_and_min_agree", [](Frame& f) { f.a.view_step = nullptr; f.a.min_agree = 32; }},
    {"same_ref_and_invalid_differs", [](Frame& f) {
         for (int j = f.gs[1]; j < f.gs[2]; j++) {
             P(j).ref = 0;
             P(j).other = 1 + (j - f.gs[1]);
             P(j).params.invalid = 0;
         }
     }},
    {"invalid_and_scale", [](Frame& f) {
         for (int j = f.gs[1]; j < f.gs[2]; j++) { P(j).params.invalid = 0; P(j).baseline = 0.1; }
         if (f.a.unit_baseline) f.unit[1] = 0.1;
     }},
    {"scale_and_geometry", [](Frame& f) {
         if (f.a.unit_baseline) f.unit[2] = 0.1;
         else for (int j = f.gs[2]; j < f.gs[3]; j++) P(j).baseline = 0.1;
         f.vs[5] = -2;
     }},
    {"geometry_and_max_diff", [](Frame& f) { f.vs[5] = -2; f.a.max_diff = -1; }},
    {"max_diff_and_max_conflict", [](Frame& f) { f.a.max_diff = -1; f.a.max_conflict = 32; }},
    {"min_agree_and_max_conflict", [](Frame& f) { f.a.min_agree = 32; f.a.max_conflict = 32; }},
    // the flag off: the check's fields are not looked at
    {"not_checked", [](Frame& f) { f.a.cross = false; f.a.view_step = nullptr; f.a.min_agree = 99; }},
};

int main() {
    // kind: 0 GROUPS sub 0, 1 GROUPS sub 1, 2 GROUPS_MIXED sub 0, 3 GROUPS_MIXED sub 1
    for (int kind = 0; kind < 4; kind++)
        for (const Case& c : kCases) {
            Frame f(kind >= 2, kind & 1);
            c.mutate(f);
            report(c.name, kind, f.a);
        }
    Frame g32(32, 16), g33(33, 16);
    report("groups_32", 0, g32.a);
    report("groups_33", 0, g33.a);
    Frame g33n(33, 16);
    g33n.a.view_step = nullptr;
    report("null_view_step_and_groups_33", 0, g33n.a);
    Frame g33s(33, 16);
    for (int j = g33s.gs[1]; j < g33s.gs[2]; j++) g33s.pairs[j].ref = 0;
    report("groups_33_and_same_ref", 0, g33s.a);
    Frame edge(3, 255), past(3, 256), low(3, -253), below(3, -254);
    report("step_255", 0, edge.a);
    report("step_256", 0, past.a);
    report("step_minus_255", 0, low.a);
    report("step_minus_256", 0, below.a);
    Frame past2(3, 256);
    past2.a.min_agree = 32;
    report("step_256_and_min_agree", 0, past2.a);
    // two reference cameras at one position, geometry consistent: views (0,0), (-1,0), (0,0)
    Frame twin(2, 0);
    twin.vs = {0, 0, -1, 0, 0, 0};
    twin.pairs[1].ref = 2;
    twin.pairs[1].other = 1;
    twin.pairs[1].params.dir = -1;
    twin.finish(false, 0);
    report("twin_position", 0, twin.a);
    twin.a.max_diff = -1;
    report("twin_position_and_max_diff", 0, twin.a);
    return 0;
}
"""

NEEDS_GROUPS = ("the cross-view check needs a group route: the pair route's maps share one "
                "reference camera")
RANGE = "view_step components must be -255..255"
# (case, status, message): one broken rule each, then two, the first in array_args.h's order
RULES = [
    ("valid", OK, ""),
    ("pair_route", UNSUPPORTED, NEEDS_GROUPS),
    ("null_view_step", INVALID, "null view_step"),
    ("same_ref", INVALID, "groups 0 and 1 share ref"),
    ("invalid_differs", INVALID, "params.invalid of group 1 differs from group 0's"),
    ("scale_differs", INVALID, "the depth scale of group 1 differs from group 0's"),
    ("geometry_sign", INVALID, "the step of pair 0 contradicts view_step"),
    ("max_diff_negative", INVALID, "max_diff must be >= 0"),
    ("max_diff_huge", OK, ""),
    ("min_agree_32", INVALID, "min_agree must be 0..31"),
    ("min_agree_negative", INVALID, "min_agree must be 0..31"),
    ("min_agree_31", OK, ""),
    ("max_conflict_32", INVALID, "max_conflict must be 0..31"),
    ("max_conflict_negative", INVALID, "max_conflict must be 0..31"),
    ("max_conflict_31", OK, ""),
    ("lr_check_and_null_view_step", UNSUPPORTED, "the multi-baseline route has no L/R check"),
    ("bad_pair_and_pair_route", INVALID, "bad pair 0"),
    ("pair_route_and_null_view_step", UNSUPPORTED, NEEDS_GROUPS),
    ("null_view_step_and_min_agree", INVALID, "null view_step"),
    ("same_ref_and_invalid_differs", INVALID, "groups 0 and 1 share ref"),
    ("invalid_and_scale", INVALID, "params.invalid of group 1 differs from group 0's"),
    ("scale_and_geometry", INVALID, "the depth scale of group 2 differs from group 0's"),
    ("max_diff_and_max_conflict", INVALID, "max_diff must be >= 0"),
    ("min_agree_and_max_conflict", INVALID, "min_agree must be 0..31"),
    ("not_checked", OK, ""),
]
LINE_RULES = [
    ("groups_32", OK, ""),
    ("groups_33", UNSUPPORTED, "the cross-view check takes 1..32 groups"),
    ("null_view_step_and_groups_33", INVALID, "null view_step"),
    ("groups_33_and_same_ref", UNSUPPORTED, "the cross-view check takes 1..32 groups"),
    ("step_255", OK, ""),
    ("step_256", INVALID, RANGE),
    ("step_minus_255", OK, ""),
    ("step_minus_256", INVALID, RANGE),
    ("step_256_and_min_agree", INVALID, RANGE),
    ("twin_position", INVALID, "two views have the same view_step"),
    ("twin_position_and_max_diff", INVALID, "two views have the same view_step"),
]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    exe = build(tmp_path_factory.mktemp("crossargs"), "crossargs", ARGS_PROGRAM)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    out = {}
    for line in run.stdout.splitlines():
        name, kind, status, msg = line.split("|", 3)
        out[(name, int(kind))] = (int(status), msg)
    return out


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("case,status,msg", RULES)
def test_rule(answers, case, status, msg, kind):
    assert answers[(case, kind)] == (status, msg)


@pytest.mark.parametrize("case,status,msg", LINE_RULES)
def test_line_frame_rule(answers, case, status, msg):
    assert answers[(case, 0)] == (status, msg)


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_geometry_rule_names_the_pair(answers, kind):
    """View 2 moved to (0, -2): the pairs that touch it contradict their steps,
    the first of them in pair order is named; with a bad threshold too, the
    geometry still answers first."""
    st, msg = answers[("geometry", kind)]
    assert st == INVALID and msg == "the step of pair 1 contradicts view_step"
    assert answers[("geometry_and_max_diff", kind)] == (st, msg)


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_subpix_needs_sub(answers, kind):
    """sub = 0 with a subpix plane is refused; sub = 1 takes a null one."""
    exp = (OK, "") if kind & 1 else (INVALID, "subpix needs sub = 1")
    assert answers[("subpix_without_sub", kind)] == exp
