"""The array frame's argument checks (csrc/array_args.h) without
a GPU.  The header -- plain C++, the one multi.cpp compiles -- is built into a
host program under AddressSanitizer and UBSan.  The program builds a valid
two-group frame for each of the four routes (sva_array_depth, _conf, _mb,
_mixed), breaks one rule at a time, and prints what check_array_args answers;
the statuses and message texts expected here are those of the two earlier
copies of these checks.  Every array of a frame is a heap array of exactly its
length, so a read through a bad group_start is a sanitizer report."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereovisionarray_amd", "csrc")
INC = os.path.join(ROOT, "include")

OK, INVALID, UNSUPPORTED = 0, 1, 2
DEPTH, CONF, MB, MIXED = 0, 1, 2, 3
ALL = (DEPTH, CONF, MB, MIXED)
PAIR, GROUP = (DEPTH, CONF), (MB, MIXED)

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include "array_args.h"
using namespace sva;

// A frame whose arrays are heap arrays of exactly their length.
struct Frame {
    int n_images, n_pairs, n_groups;
    std::unique_ptr<uint8_t[]> pixel{new uint8_t[1]()};
    std::unique_ptr<const uint8_t*[]> images;
    std::unique_ptr<sva_array_pair[]> pairs;
    std::unique_ptr<int32_t[]> gs;
    std::unique_ptr<double[]> unit, depth{new double[1]()};
    std::unique_ptr<uint8_t[]> winner{new uint8_t[1]()};
    ArrayArgs a;

    // route: 0 sva_array_depth, 1 _conf, 2 _mb, 3 _mixed.  Every group: one
    // reference view (g mod 3) against the other two of the first three views
    // in turn; the fourth view belongs to no pair.
    Frame(int route, int n_pairs_, std::initializer_list<int> starts, int n_images_ = 4)
        : n_images(n_images_), n_pairs(n_pairs_), n_groups((int)starts.size() - 1),
          images(new const uint8_t*[n_images_]), pairs(new sva_array_pair[n_pairs_]),
          gs(new int32_t[starts.size()]), unit(new double[starts.size() - 1]) {
        for (int v = 0; v < n_images; v++) images[v] = pixel.get();
        int k = 0;
        for (int s : starts) gs[k++] = s;
        for (int g = 0; g < n_groups; g++) unit[g] = 0.05;
        for (int j = 0; j < n_pairs; j++) {
            sva_array_pair& q = pairs[j];
            std::memset(&q, 0, sizeof q);
            int g = 0;
            while (g + 1 < n_groups && j >= gs[g + 1] && gs[g + 1] > gs[g]) g++;
            q.ref = g % 3;
            q.other = (q.ref + 1 + j % 2) % 3;
            q.params.D = 64;
            q.params.dir = 1;
            q.params.P1 = 10;
            q.params.P2 = 120;
            q.params.invalid = 0xffff;
            q.baseline = 0.05;
        }
        a.images = images.get();
        a.n_images = n_images;
        a.W = 20;
        a.H = 20;
        a.pitch = 20;
        a.pairs = pairs.get();
        a.n_pairs = n_pairs;
        a.group_start = gs.get();
        a.n_groups = n_groups;
        a.f = 0.05;
        a.pixel_size = 1e-5;
        a.depth = depth.get();
        a.route = route < 2 ? ArrayRoute::Pairs : route == 2 ? ArrayRoute::Groups
                                                             : ArrayRoute::GroupsMixed;
        a.conf = route != 0;
        a.mode = route == 1 ? SVA_FUSE_MIN_COST : SVA_FUSE_MEDIAN;
        if (route == 3) {
            a.unit_baseline = unit.get();
            if (n_pairs > 1 && gs[1] > 1) pairs[1].baseline = 0.1;   // 2/1 of the unit
        }
    }
};

struct Case {
    const char* name;
    void (*mutate)(Frame&);
};
#define P(j) f.pairs[j]
const Case kCases[] = {
    {"valid", [](Frame&) {}},
    // 1. the route's options
    {"mode", [](Frame& f) { f.a.mode = 7; }},
    {"uniqueness_high", [](Frame& f) { f.a.uniqueness = 101; }},
    {"uniqueness_low", [](Frame& f) { f.a.uniqueness = -1; }},
    {"winner_median", [](Frame& f) { f.a.mode = SVA_FUSE_MEDIAN; f.a.winner = f.winner.get(); }},
    {"null_unit", [](Frame& f) { f.a.unit_baseline = nullptr; }},
    // 2. sizes and pointers
    {"null_images", [](Frame& f) { f.a.images = nullptr; }},
    {"no_images", [](Frame& f) { f.a.n_images = 0; }},
    {"null_pairs", [](Frame& f) { f.a.pairs = nullptr; }},
    {"no_pairs", [](Frame& f) { f.a.n_pairs = 0; }},
    {"null_group_start", [](Frame& f) { f.a.group_start = nullptr; }},
    {"no_groups", [](Frame& f) { f.a.n_groups = 0; }},
    {"null_depth", [](Frame& f) { f.a.depth = nullptr; }},
    {"zero_width", [](Frame& f) { f.a.W = 0; }},
    {"zero_height", [](Frame& f) { f.a.H = 0; }},
    {"short_pitch", [](Frame& f) { f.a.pitch = 19; }},
    // 3. the ends of group_start
    {"start_not_zero", [](Frame& f) { f.gs[0] = 1; }},
    {"end_not_n_pairs", [](Frame& f) { f.gs[f.n_groups] = f.n_pairs - 1; }},
    // 4. group sizes
    {"empty_group", [](Frame& f) { f.gs[1] = 0; }},
    // 5. per pair
    {"ref_negative", [](Frame& f) { P(3).ref = -1; }},
    {"ref_past_end", [](Frame& f) { P(3).ref = f.n_images; }},
    {"other_negative", [](Frame& f) { P(3).other = -1; }},
    {"other_past_end", [](Frame& f) { P(3).other = f.n_images; }},
    {"null_image", [](Frame& f) { P(3).other = 3; f.images[3] = nullptr; }},
    {"D_zero", [](Frame& f) { P(3).params.D = 0; }},
    {"D_257", [](Frame& f) { P(3).params.D = 257; }},
    {"dmin_negative", [](Frame& f) { P(3).params.dmin = -1; }},
    {"zero_step", [](Frame& f) { P(3).params.dir = 0; }},
    {"lr_check", [](Frame& f) { P(3).params.lr_check = 1; }},
    // 6. per group
    {"invalid_differs", [](Frame& f) { P(3).params.invalid = 0; }},
    {"ref_differs", [](Frame& f) { P(3).ref = 2; P(3).other = 0; }},
    {"D_differs", [](Frame& f) { P(3).params.D = 128; }},
    {"dmin_differs", [](Frame& f) { P(3).params.dmin = 1; }},
    {"P1_differs", [](Frame& f) { P(3).params.P1 = 11; }},
    {"P2_differs", [](Frame& f) { P(3).params.P2 = 121; }},
    {"baseline_differs", [](Frame& f) { P(3).baseline = 0.1; }},
    // 7. the mixed route's ratios
    {"ratio_9", [](Frame& f) { P(3).baseline = 0.45; }},
    {"ratio_irrational", [](Frame& f) { P(3).baseline = 0.0707; }},
    {"unit_zero", [](Frame& f) { f.unit[1] = 0; }},
    {"distance", [](Frame& f) { P(2).params.dmin = P(3).params.dmin = 65500; }},
    {"distance_huge", [](Frame& f) { P(2).params.dmin = P(3).params.dmin = 0x7fffffff - 10; }},
    {"distance_fits", [](Frame& f) { P(2).params.dmin = P(3).params.dmin = 65535 - 63; }},
    // several rules at once: the first in the documented order
    {"bad_pair_and_invalid_differs", [](Frame& f) { P(3).ref = -1; P(1).params.invalid = 0; }},
    {"empty_group_and_bad_pair", [](Frame& f) { f.gs[1] = 0; P(0).ref = -1; }},
    {"uniqueness_and_null_images", [](Frame& f) { f.a.uniqueness = 101; f.a.images = nullptr; }},
};

void report(const char* name, int route, const ArrayArgs& a) {
    std::string msg;
    std::vector<int32_t> ratio;
    const int st = check_array_args(a, msg, ratio);
    std::printf("%s|%d|%d|%s\n", name, route, st, msg.c_str());
}

int gcd(int a, int b) { return b ? gcd(b, a % b) : a; }

int main() {
    for (int route = 0; route < 4; route++) {
        for (const Case& c : kCases) {
            Frame f(route, 4, {0, 2, 4});
            c.mutate(f);
            report(c.name, route, f.a);
        }
        // group_start = {0, 20, 10} over 10 pairs: the ends pass, group 0 has 20
        // pairs (within 1..32), pairs[10..19] do not exist
        Frame back(route, 10, {0, 20, 10});
        report("group_start_goes_back", route, back.a);
        Frame big(route, 34, {0, 33, 34});
        report("group_of_33", route, big.a);
        Frame full(route, 33, {0, 32, 33});
        report("group_of_32", route, full.a);
    }
    // the mixed route's ratio table: pair 1 of the valid frame is at 2/1
    {
        Frame f(3, 4, {0, 2, 4});
        std::string msg;
        std::vector<int32_t> r;
        const int st = check_array_args(f.a, msg, r);
        std::printf("ratios|3|%d|", st);
        for (int32_t v : r) std::printf("%d ", v);
        std::printf("\n");
    }
    // baseline_ratio against brute force: every num/den in 1..8 over a few units
    // comes back reduced; nothing else is a ratio
    int bad = 0, n = 0;
    const double units[] = {0.05, 1.0, 0.0375, 1e-3, 123.456, 3.0};
    for (double u : units) {
        for (int num = 1; num <= 8; num++)
            for (int den = 1; den <= 8; den++, n++) {
                const int g = gcd(num, den);
                int32_t rn = 0, rd = 0;
                if (!baseline_ratio(u * num / den, u, &rn, &rd) || rn != num / g || rd != den / g) {
                    std::printf("baseline_ratio_bad|%d|1|%g: %d/%d -> %d/%d\n", n, u, num, den, rn, rd);
                    bad++;
                }
            }
        int32_t rn, rd;
        for (double b : {9 * u, u / 9, 8.5 * u, u * 0.7071, 0.0, -u, u * (1 + 1e-6)})
            if (baseline_ratio(b, u, &rn, &rd)) {
                std::printf("baseline_ratio_bad|%d|1|%g: %g accepted\n", n, u, b);
                bad++;
            }
        if (baseline_ratio(u, 0.0, &rn, &rd) || baseline_ratio(u, -u, &rn, &rd)) bad++;
    }
    std::printf("baseline_ratio_checked|%d|%d|\n", n, bad);
    return 0;
}
"""


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """{(case, route): (status, message)} as the program printed them; the
    sanitizers abort the program on any finding."""
    d = tmp_path_factory.mktemp("arrayargs")
    src = d / "arrayargs.cpp"
    src.write_text(PROGRAM)
    exe = d / "arrayargs"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-g", "-I", CSRC, "-I", INC, str(src), "-o",
                    str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    out = {}
    for line in run.stdout.splitlines():
        name, route, status, msg = line.split("|", 3)
        out[(name, int(route))] = (int(status), msg)
    return out


@pytest.mark.parametrize("route", ALL)
def test_valid_frame_passes(answers, route):
    assert answers[("valid", route)] == (OK, "")
    assert answers[("group_of_32", route)] == (OK, "")
    assert answers[("distance_fits", route)] == (OK, "")


BAD_ARGS = ["null_images", "no_images", "null_pairs", "no_pairs", "null_group_start", "no_groups",
            "null_depth", "zero_width", "zero_height", "short_pitch"]
BAD_PAIR = ["ref_negative", "ref_past_end", "other_negative", "other_past_end", "null_image",
            "D_zero", "D_257", "dmin_negative", "zero_step"]
SHARE = "the pairs of group 1 must share D, dmin, P1, P2 and invalid"
NO_RATIO = "the baseline of pair 3 is no num/den (1..8 each) of its group's unit baseline"

# (case, the routes it is a rule of, status, message): one broken rule each
RULES = [
    ("mode", (CONF,), INVALID, "unknown fusion mode"),
    ("uniqueness_high", (CONF, MB, MIXED), INVALID, "uniqueness must be 0..100"),
    ("uniqueness_low", (CONF, MB, MIXED), INVALID, "uniqueness must be 0..100"),
    ("winner_median", (CONF,), INVALID, "the median has no winner map"),
    ("null_unit", (MIXED,), INVALID, "null unit_baseline"),
] + [(c, ALL, INVALID, "bad array arguments") for c in BAD_ARGS] + [
    ("start_not_zero", ALL, INVALID, "group_start must run from 0 to n_pairs"),
    ("end_not_n_pairs", ALL, INVALID, "group_start must run from 0 to n_pairs"),
    ("empty_group", ALL, UNSUPPORTED, "groups of 1..32 pairs"),
    ("group_of_33", ALL, UNSUPPORTED, "groups of 1..32 pairs"),
] + [(c, ALL, INVALID, "bad pair 3") for c in BAD_PAIR] + [
    ("lr_check", GROUP, UNSUPPORTED, "the multi-baseline route has no L/R check"),
    ("invalid_differs", PAIR, INVALID, "params.invalid differs within group 1"),
    ("invalid_differs", GROUP, INVALID, SHARE),
    ("ref_differs", GROUP, INVALID, "the pairs of group 1 do not share ref"),
    ("D_differs", GROUP, INVALID, SHARE),
    ("dmin_differs", GROUP, INVALID, SHARE),
    ("P1_differs", GROUP, INVALID, SHARE),
    ("P2_differs", GROUP, INVALID, SHARE),
    ("baseline_differs", (MB,), INVALID, "the pairs of group 1 have different major-axis baselines"),
    ("ratio_9", (MIXED,), INVALID, NO_RATIO),
    ("ratio_irrational", (MIXED,), INVALID, NO_RATIO),
    ("unit_zero", (MIXED,), INVALID,
     "the baseline of pair 2 is no num/den (1..8 each) of its group's unit baseline"),
    ("distance", (MIXED,), INVALID, "the match distance of pair 2 exceeds 16 bits"),
    ("distance_huge", (MIXED,), INVALID, "the match distance of pair 2 exceeds 16 bits"),
]


@pytest.mark.parametrize("case,routes,status,message", RULES,
                         ids=["%s-%s" % (r[0], "".join(map(str, r[1]))) for r in RULES])
def test_one_broken_rule(answers, case, routes, status, message):
    for route in routes:
        assert answers[(case, route)] == (status, message), route


def test_a_rule_of_another_route_is_no_rule(answers):
    """What only some routes refuse, the others accept."""
    for case, routes in [("lr_check", PAIR), ("ref_differs", PAIR), ("D_differs", PAIR),
                         ("baseline_differs", PAIR + (MIXED,)), ("null_unit", (DEPTH, CONF, MB)),
                         ("mode", (DEPTH,)), ("uniqueness_high", (DEPTH,)),
                         ("distance", (DEPTH, CONF, MB))]:
        for route in routes:
            assert answers[(case, route)] == (OK, ""), (case, route)


@pytest.mark.parametrize("route", ALL)
def test_group_start_that_goes_back_reads_no_pair(answers, route):
    """n_pairs = 10, group_start = {0, 20, 10}: refused on the group sizes, and
    pairs[10..19] -- past the heap array of exactly 10 -- are never read (the
    sanitizer would have ended the program)."""
    assert answers[("group_start_goes_back", route)] == (UNSUPPORTED, "groups of 1..32 pairs")


def test_several_broken_rules_report_the_first_in_order(answers):
    for route in PAIR:
        assert answers[("bad_pair_and_invalid_differs", route)] == (INVALID, "bad pair 3")
    for route in ALL:
        assert answers[("empty_group_and_bad_pair", route)] == (UNSUPPORTED,
                                                                "groups of 1..32 pairs")
    for route in (CONF, MB, MIXED):
        assert answers[("uniqueness_and_null_images", route)] == (INVALID,
                                                                  "uniqueness must be 0..100")


def test_mixed_route_returns_the_reduced_ratios(answers):
    assert answers[("ratios", MIXED)] == (OK, "1 1 2 1 1 1 1 1 ")


def test_baseline_ratio_equals_brute_force(answers):
    """Every num/den in 1..8 over six units comes back reduced; 9/1, 1/9, 17/2,
    an irrational, zero, a negative and a 1e-6 miss are refused."""
    assert answers[("baseline_ratio_checked", 6 * 64)] == (0, "")
