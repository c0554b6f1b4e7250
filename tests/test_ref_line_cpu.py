"""Mode R's line arithmetic (csrc/ref_line.h) and launch plan (csrc/ref_plan.h)
without a GPU.  The two headers -- plain C++, the ones refpath.hip compiles --
are built into a host program under AddressSanitizer and UBSan that answers
the queries below.  What is expected of it comes from elsewhere: the reference's
own Bresenham output (tests/golden/ref_bresenham.npz), a transcription of the
reference's iterative plotLineLow / plotLineHigh (functions.cpp:253-321) that
is itself held to that fixture, and the share rule as DESIGN.md §4.2 states it."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereovisionarray_amd", "csrc")
INC = os.path.join(ROOT, "include")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_ref_golden as mk  # noqa: E402

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "ref_line.h"
#include "ref_plan.h"
using namespace sva;

// One query per input line, one answer per output line:
//   pts x0 y0 x1 y1                 -> n, then line_point(make_line(..), i) for i < n
//   iv x0 y0 x1 y1 px py cm ok d..  -> lo len ib0 per outer offset d, for pixel (px, py) and
//                                      inner axis y (cm = 1) or x, packed as ref_plane3_kernel packs
//   plan W H k cu dbg               -> route gx gy shares wide key_size key_bytes
//   tune                            -> kPlaneMinBlocks kPlaneSplitMin kPlaneSplitMax kPlaneSplitRounds
int main(int argc, char** argv) {
    std::FILE* f = argc > 1 ? std::fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    char cmd[16];
    while (std::fscanf(f, "%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "pts")) {
            int x0, y0, x1, y1;
            if (std::fscanf(f, "%d %d %d %d", &x0, &y0, &x1, &y1) != 4) return 3;
            const Line L = make_line(x0, y0, x1, y1);
            std::printf("%d", L.n);
            for (int i = 0; i < L.n; i++) {
                int cx, cy;
                line_point(L, i, cx, cy);
                std::printf(" %d %d", cx, cy);
            }
            std::printf("\n");
        } else if (!std::strcmp(cmd, "iv")) {
            int x0, y0, x1, y1, px, py, cm, ok, nd;
            if (std::fscanf(f, "%d %d %d %d %d %d %d %d %d", &x0, &y0, &x1, &y1, &px, &py, &cm, &ok,
                            &nd) != 9)
                return 3;
            const Line L = make_line(x0, y0, x1, y1);
            const bool high = L.high != 0, neg = L.step < 0;
            const int ox = px - L.x0, oy = py - L.y0;
            const int po = line_po(high ? oy : ox, high ? ox : oy);
            const int pa = line_pa(L), pn = line_pn(L, ok != 0);
            for (int q = 0; q < nd; q++) {
                int d, lo, len, ib0;
                if (std::fscanf(f, "%d", &d) != 1) return 3;
                line_interval(po, pa, pn, high == (cm != 0), neg, d, lo, len, ib0);
                std::printf("%s%d %d %d", q ? " " : "", lo, len, ib0);
            }
            std::printf("\n");
        } else if (!std::strcmp(cmd, "plan")) {
            int W, H, k, cu, dbg;
            if (std::fscanf(f, "%d %d %d %d %d", &W, &H, &k, &cu, &dbg) != 5) return 3;
            const RefMatchPlan p = ref_match_plan(W, H, k, cu, dbg);
            std::printf("%d %d %d %d %d %zu %zu\n", (int)p.route, p.gx, p.gy, p.shares, (int)p.wide,
                        p.key_size, p.key_bytes);
        } else if (!std::strcmp(cmd, "tune")) {
            std::printf("%d %d %d %d\n", tune::kPlaneMinBlocks, tune::kPlaneSplitMin,
                        tune::kPlaneSplitMax, tune::kPlaneSplitRounds);
        } else {
            return 4;
        }
    }
    std::fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    """ask(queries) -> the program's answers, one list of ints per query.  The
    sanitizers abort the program on any finding."""
    d = tmp_path_factory.mktemp("refline")
    src = d / "refline.cpp"
    src.write_text(PROGRAM)
    exe = d / "refline"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-g", "-I", CSRC, "-I", INC, str(src), "-o",
                    str(exe)], check=True)
    count = [0]

    def ask(queries):
        count[0] += 1
        q = d / ("queries%d.txt" % count[0])
        q.write_text("".join(" ".join(str(v) for v in row) + "\n" for row in queries))
        run = subprocess.run([str(exe), str(q)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stderr == "", run.stderr
        lines = run.stdout.splitlines()
        assert len(lines) == len(queries)
        return [[int(v) for v in line.split()] for line in lines]
    return ask


def bresenham(p1, p2):
    """functions.cpp:253-321, the iterative form: bresenham(p1, p2) emits from
    the end with the lower major coordinate."""
    (ax, ay), (bx, by) = p1, p2
    low = abs(ay - by) < abs(ax - bx)
    if (bx > ax) if low else (by > ay):
        x0, y0, x1, y1 = ax, ay, bx, by
    else:
        x0, y0, x1, y1 = bx, by, ax, ay
    if not low:                      # plotLineHigh is plotLineLow transposed
        x0, y0, x1, y1 = y0, x0, y1, x1
    dx, dy, step = x1 - x0, abs(y1 - y0), (-1 if y1 < y0 else 1)
    D, y, pts = 2 * dy - dx, y0, []
    for x in range(x0, x1 + 1):
        pts.append((x, y) if low else (y, x))
        if D > 0:
            y += step
            D += 2 * (dy - dx)
        else:
            D += 2 * dy
    return pts


def fixture_lines():
    fx = mk.load("ref_bresenham")
    off, pairs = fx["offsets"], mk.in_bresenham().tolist()
    assert len(off) == len(pairs) + 1 and len(pairs) >= 200
    return [(tuple(p), [tuple(q) for q in fx["points"][off[i]:off[i + 1]].tolist()])
            for i, p in enumerate(pairs)]


def test_transcription_equals_the_reference():
    """The brute force below stands on this: the Python transcription emits the
    reference's own point lists."""
    for (x0, y0, x1, y1), want in fixture_lines():
        assert bresenham((x0, y0), (x1, y1)) == want, (x0, y0, x1, y1)


def test_line_point_equals_the_reference(ask):
    """line_point(make_line(p1, p2), i), i < n, is the reference's list in order,
    for every endpoint pair of the fixture."""
    lines = fixture_lines()
    got = ask([("pts",) + p for p, _ in lines])
    for (p, want), g in zip(lines, got):
        assert g[0] == len(want), p
        assert list(zip(g[1::2], g[2::2])) == want, p


def check_intervals(ask, cases, whole=False):
    """cases: (a, b, pixel, cm, outer offsets).  The interval of every outer
    offset is exactly the set of inner offsets among {c_i - pixel} there, and
    d_in + ib0 is the candidate's index; with `whole`, the outer offsets hold
    the whole line.  Returns the number of intervals."""
    got = ask([("iv",) + a + b + p + (int(cm), 1, len(ds)) + tuple(ds) for a, b, p, cm, ds in cases])
    checked = 0
    for (a, b, p, cm, ds), g in zip(cases, got):
        at = {}                                  # outer offset -> {inner offset: i}
        pts = bresenham(a, b)
        for i, (cx, cy) in enumerate(pts):
            dx, dy = cx - p[0], cy - p[1]
            at.setdefault(dx if cm else dy, {})[dy if cm else dx] = i
        for d, lo, ln, ib0 in zip(ds, g[0::3], g[1::3], g[2::3]):
            want = at.get(d, {})
            assert ln == len(want), (a, b, p, cm, d)
            assert sorted(want) == list(range(lo, lo + ln)), (a, b, p, cm, d)
            assert all(d_in + ib0 == i for d_in, i in want.items()), (a, b, p, cm, d)
            checked += 1
        assert not whole or sum(g[1::3]) == len(pts), (a, b, p, cm)
    return checked


def test_line_interval_brute_force(ask):
    """Every line from (1, 2) into the 19 x 19 box around it (the single point
    included), both endpoint orders, two pixels, both inner axes, outer offsets
    -15..15 -- which hold every candidate's offset, so the intervals of a line
    also cover all of it."""
    first, ds = (1, 2), list(range(-15, 16))
    cases = []
    for ex in range(-9, 10):
        for ey in range(-9, 10):
            second = (first[0] + ex, first[1] + ey)
            for a, b in ((first, second), (second, first)):
                for p in ((0, 0), (3, -2)):
                    for cm in (False, True):
                        cases.append((a, b, p, cm, ds))
    assert check_intervals(ask, cases, whole=True) == 89528


LONG_LINES = [((0, 0), (4159, 2000)), ((0, 0), (2000, 4159)), ((4159, 0), (0, 2000)),
              ((0, 4159), (2000, 0)), ((20, 20), (4139, 4139)), ((20, 31), (4139, 31)),
              ((0, 0), (32766, 30001)), ((30001, 0), (0, 32766))]


def test_line_interval_long_lines(ask):
    """Lines at the scale of a 4160-pixel frame, and of the largest frame the
    API accepts, both directions: the products and the 16-bit halves under
    UBSan.  Outer offsets sampled, the line's ends and far outside included --
    for the largest lines only offsets that some point of the line has, where
    ref_line.h states that its int products fit."""
    cases = []
    for a, b in LONG_LINES:
        span = max(abs(a[0] - b[0]), abs(a[1] - b[1]))
        for a_, b_ in ((a, b), (b, a)):
            for p in ((100, 50), (min(span, 4000), min(span, 1990))):
                for cm in (False, True):
                    ds = sorted(set(range(-span - 40, span + 41, max(37, span // 150))) |
                                {-span - 1, -span, -1, 0, 1, span - 1, span, span + 1})
                    if span > 16383:
                        own = {c[0 if cm else 1] - p[0 if cm else 1] for c in bresenham(a, b)}
                        ds = [d for d in ds if d in own] + [min(own), max(own)]
                    cases.append((a_, b_, p, cm, ds))
    assert check_intervals(ask, cases) > 8000
    # a pixel that takes no part (n = 0 in pn) has no interval anywhere
    a, b = LONG_LINES[0]
    ds = list(range(-4200, 4201, 100))
    for g in ask([("iv",) + a + b + (100, 50, cm, 0, len(ds)) + tuple(ds) for cm in (0, 1)]):
        assert not any(g[1::3])
    # and the points of the long lines are the transcription's
    got = ask([("pts",) + a + b for a, b in LONG_LINES])
    for (a, b), g in zip(LONG_LINES, got):
        assert list(zip(g[1::2], g[2::2])) == bresenham(a, b), (a, b)


# ---------------------------------------------------------------- the plan --
NONE, PIXEL, PLANE = 0, 1, 2
FRAMES = [(1920, 1080), (3840, 2160), (2560, 1440), (1280, 720), (640, 480), (960, 540),
          (4160, 2340), (129, 97), (8192, 70)]


def ceil_div(a, b):
    return -(-a // b)


def shares_rule(tiles, cu, tune):
    """DESIGN.md §4.2, every tile split: about kPlaneSplitRounds rounds of the
    chip's workgroup slots (kPlaneMinBlocks per CU) over the tile count,
    rounded, within [kPlaneSplitMin, kPlaneSplitMax]."""
    min_blocks, smin, smax, rounds = tune
    slots = cu * min_blocks
    if slots <= 0 or tiles <= 0:
        return 1
    return max(smin, min(smax, (rounds * slots + tiles // 2) // tiles))


def test_plan_grid_and_shares(ask):
    tune = ask([("tune",)])[0]
    queries = [(W, H, k, cu) for W, H in FRAMES for k in (1, 8, 20, 32) for cu in (256, 64, 0)]
    got = ask([("plan",) + q + (0,) for q in queries])
    for (W, H, k, cu), (route, gx, gy, shares, wide, ksize, kbytes) in zip(queries, got):
        assert (route, gx, gy) == (PLANE, ceil_div(W - 2 * k, 64), ceil_div(H - 2 * k, 32))
        assert shares == shares_rule(gx * gy, cu, tune), (W, H, k, cu)
        assert wide == (W >= 4096 or H >= 4096) and ksize == (8 if wide else 4)
        assert kbytes == (W * H * ksize if shares > 1 else 0)


def test_plan_shipped_table(ask):
    """The table of DESIGN.md §4.2 at 256 CUs and k = 20, literally: a change of
    the tuning constants has to change this test too."""
    assert ask([("tune",)])[0] == [3, 3, 6, 4]   # min blocks per CU, shares min / max, rounds
    table = {(1920, 1080): (30, 33, 3), (3840, 2160): (60, 67, 3), (2560, 1440): (40, 44, 3),
             (1280, 720): (20, 22, 6), (640, 480): (10, 14, 6)}
    plans = ask([("plan", W, H, 20, 256, 0) for W, H in table])
    for want, p in zip(table.values(), plans):
        assert p[0] == PLANE and tuple(p[1:4]) == want
    assert 30 * 33 == 990


def test_plan_forced_shares(ask):
    """SVA_DEBUG_PLANE_SPLIT 1..16 sets the share count; 0 and 17 do not."""
    tune = ask([("tune",)])[0]
    ruled = shares_rule(30 * 33, 256, tune)
    got = ask([("plan", 1920, 1080, 20, 256, dbg) for dbg in (-1, 0, 1, 2, 7, 16, 17)])
    assert [p[3] for p in got] == [ruled, ruled, 1, 2, 7, 16, ruled]
    assert [p[6] for p in got] == [1920 * 1080 * 4 if p[3] > 1 else 0 for p in got]
    assert got[2][5:] == [4, 0]                     # one share: no key buffer
    wide1, wide5 = ask([("plan", 4160, 2340, 20, 256, dbg) for dbg in (1, 5)])
    assert wide1[4:] == [1, 8, 0] and wide5[4:] == [1, 8, 4160 * 2340 * 8]


def test_plan_routes(ask):
    got = ask([("plan", 640, 480, 32, 256, 0), ("plan", 640, 480, 33, 256, 0),
               ("plan", 640, 480, 33, 256, 5), ("plan", 640, 480, 100, 256, 0),
               ("plan", 40, 480, 20, 256, 0), ("plan", 480, 40, 20, 256, 0),
               ("plan", 30, 30, 20, 256, 0), ("plan", 41, 41, 20, 256, 0)])
    assert got[0][0] == PLANE
    # k > 32: one wave per pixel, four pixels per workgroup, no shares and no keys
    assert got[1] == [PIXEL, ceil_div(640 - 66, 4), 480 - 66, 1, 0, 4, 0]
    assert got[2] == got[1] and got[3] == [PIXEL, 110, 280, 1, 0, 4, 0]
    # W - 2k <= 0 or H - 2k <= 0: nothing to do
    assert [g[0] for g in got[4:7]] == [NONE] * 3 and all(g[6] == 0 for g in got[4:7])
    assert got[7][:3] == [PLANE, 1, 1]


def test_plan_wide(ask):
    """u64 keys exactly when W or H >= 4096."""
    got = ask([("plan", 4095, 4095, 20, 256, 0), ("plan", 4096, 8, 2, 256, 0),
               ("plan", 8, 4096, 2, 256, 0), ("plan", 4096, 4096, 40, 256, 0)])
    assert [g[4] for g in got] == [0, 1, 1, 1]
    assert [g[5] for g in got] == [4, 8, 8, 8]
    assert got[0][6] == 4095 * 4095 * 4 and got[1][6] == 4096 * 8 * 8 and got[3][6] == 0
