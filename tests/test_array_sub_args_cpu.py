"""sva_array_depth_sub's argument checks (csrc/array_args.h) without
a GPU, in the manner of tests/test_array_args_cpu.py: the header is built into a
host program under AddressSanitizer and UBSan.  The program builds a valid
two-group frame for the four old entries and for the new entry's three routes,
breaks one rule at a time and prints what check_array_args answers.  Checked
here: every new refusal; that the route's options are refused before a bad
group_start is read (every array is a heap array of exactly its length, so a
read through it is a sanitizer report); and that the four old routes answer
every case of tests/test_array_args_cpu.py as that file expects."""
import os
import subprocess

import pytest

import test_array_args_cpu as old

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereovisionarray_amd", "csrc")
INC = os.path.join(ROOT, "include")

OK, INVALID, UNSUPPORTED = 0, 1, 2
DEPTH, CONF, MB, MIXED, SUB_PAIRS, SUB_GROUPS, SUB_MIXED = range(7)
OLD = (DEPTH, CONF, MB, MIXED)
SUB = (SUB_PAIRS, SUB_GROUPS, SUB_MIXED)
SUB_GROUP = (SUB_GROUPS, SUB_MIXED)
# the old entry whose rules a route of the new entry shares
LIKE = {SUB_PAIRS: CONF, SUB_GROUPS: MB, SUB_MIXED: MIXED}

GROUP_MODE = "the group routes fuse one map: SVA_FUSE_MEDIAN only"
GROUP_PLANES = "the group routes have no n_valid or winner map"
UNIT_ELSEWHERE = "unit_baseline is for SVA_ARRAY_GROUPS_MIXED only"

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include "array_args.h"
using namespace sva;

// A frame whose arrays are heap arrays of exactly their length.  entry: 0
// sva_array_depth, 1 _conf, 2 _mb, 3 _mixed, 4..6 sva_array_depth_sub with
// SVA_ARRAY_PAIRS, _GROUPS, _GROUPS_MIXED.
struct Frame {
    int n_images, n_pairs, n_groups;
    std::unique_ptr<uint8_t[]> pixel{new uint8_t[1]()};
    std::unique_ptr<const uint8_t*[]> images;
    std::unique_ptr<sva_array_pair[]> pairs;
    std::unique_ptr<int32_t[]> gs;
    std::unique_ptr<double[]> unit, depth{new double[1]()};
    std::unique_ptr<uint8_t[]> winner{new uint8_t[1]()}, n_valid{new uint8_t[1]()};
    std::unique_ptr<float[]> subpix{new float[1]()};
    ArrayArgs a;

    Frame(int entry, int n_pairs_, std::initializer_list<int> starts, int n_images_ = 4)
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
        if (entry < 4) {
            a.route = entry < 2 ? ArrayRoute::Pairs : entry == 2 ? ArrayRoute::Groups
                                                                 : ArrayRoute::GroupsMixed;
            a.conf = entry != 0;
            a.mode = entry == 1 ? SVA_FUSE_MIN_COST : SVA_FUSE_MEDIAN;
        } else {
            a.route = array_route_of(entry - 4);
            a.conf = true;
            a.sub = true;
            a.mode = SVA_FUSE_MEDIAN;
            a.subpix = subpix.get();
        }
        if (a.route == ArrayRoute::GroupsMixed) {
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
    // the cases of tests/test_array_args_cpu.py
    {"valid", [](Frame&) {}},
    {"mode", [](Frame& f) { f.a.mode = 7; }},
    {"uniqueness_high", [](Frame& f) { f.a.uniqueness = 101; }},
    {"uniqueness_low", [](Frame& f) { f.a.uniqueness = -1; }},
    {"winner_median", [](Frame& f) { f.a.mode = SVA_FUSE_MEDIAN; f.a.winner = f.winner.get(); }},
    {"null_unit", [](Frame& f) { f.a.unit_baseline = nullptr; }},
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
    {"start_not_zero", [](Frame& f) { f.gs[0] = 1; }},
    {"end_not_n_pairs", [](Frame& f) { f.gs[f.n_groups] = f.n_pairs - 1; }},
    {"empty_group", [](Frame& f) { f.gs[1] = 0; }},
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
    {"invalid_differs", [](Frame& f) { P(3).params.invalid = 0; }},
    {"ref_differs", [](Frame& f) { P(3).ref = 2; P(3).other = 0; }},
    {"D_differs", [](Frame& f) { P(3).params.D = 128; }},
    {"dmin_differs", [](Frame& f) { P(3).params.dmin = 1; }},
    {"P1_differs", [](Frame& f) { P(3).params.P1 = 11; }},
    {"P2_differs", [](Frame& f) { P(3).params.P2 = 121; }},
    {"baseline_differs", [](Frame& f) { P(3).baseline = 0.1; }},
    {"ratio_9", [](Frame& f) { P(3).baseline = 0.45; }},
    {"ratio_irrational", [](Frame& f) { P(3).baseline = 0.0707; }},
    {"unit_zero", [](Frame& f) { f.unit[1] = 0; }},
    {"distance", [](Frame& f) { P(2).params.dmin = P(3).params.dmin = 65500; }},
    {"distance_huge", [](Frame& f) { P(2).params.dmin = P(3).params.dmin = 0x7fffffff - 10; }},
    {"distance_fits", [](Frame& f) { P(2).params.dmin = P(3).params.dmin = 65535 - 63; }},
    {"bad_pair_and_invalid_differs", [](Frame& f) { P(3).ref = -1; P(1).params.invalid = 0; }},
    {"empty_group_and_bad_pair", [](Frame& f) { f.gs[1] = 0; P(0).ref = -1; }},
    {"uniqueness_and_null_images", [](Frame& f) { f.a.uniqueness = 101; f.a.images = nullptr; }},
    // the new entry's options
    {"unknown_route", [](Frame& f) { f.a.route = array_route_of(3); }},
    {"negative_route", [](Frame& f) { f.a.route = array_route_of(-1); }},
    {"min_cost", [](Frame& f) { f.a.mode = SVA_FUSE_MIN_COST; }},
    {"max_margin", [](Frame& f) { f.a.mode = SVA_FUSE_MAX_MARGIN; }},
    {"min_cost_planes", [](Frame& f) { f.a.mode = SVA_FUSE_MIN_COST; f.a.winner = f.winner.get();
                                       f.a.n_valid = f.n_valid.get(); }},
    {"n_valid", [](Frame& f) { f.a.n_valid = f.n_valid.get(); }},
    {"unit_given", [](Frame& f) { f.a.unit_baseline = f.unit.get(); }},
    {"no_subpix", [](Frame& f) { f.a.subpix = nullptr; }},
    // several at once: the first in the documented order
    {"unknown_route_and_null_group_start",
     [](Frame& f) { f.a.route = array_route_of(9); f.a.group_start = nullptr; }},
    {"uniqueness_and_min_cost", [](Frame& f) { f.a.uniqueness = 101; f.a.mode = SVA_FUSE_MIN_COST; }},
    {"min_cost_and_n_valid", [](Frame& f) { f.a.mode = SVA_FUSE_MIN_COST;
                                            f.a.n_valid = f.n_valid.get(); }},
    {"n_valid_and_null_images", [](Frame& f) { f.a.n_valid = f.n_valid.get(); f.a.images = nullptr; }},
    {"unit_given_and_empty_group", [](Frame& f) { f.a.unit_baseline = f.unit.get(); f.gs[1] = 0; }},
};

void report(const char* name, int entry, const ArrayArgs& a) {
    std::string msg;
    std::vector<int32_t> ratio;
    const int st = check_array_args(a, msg, ratio);
    std::printf("%s|%d|%d|%s\n", name, entry, st, msg.c_str());
}

int main() {
    for (int entry = 0; entry < 7; entry++) {
        for (const Case& c : kCases) {
            Frame f(entry, 4, {0, 2, 4});
            c.mutate(f);
            report(c.name, entry, f.a);
        }
        // group_start = {0, 20, 10} over 10 pairs: the ends pass, group 0 has 20
        // pairs (within 1..32), pairs[10..19] do not exist
        Frame back(entry, 10, {0, 20, 10});
        report("group_start_goes_back", entry, back.a);
        // ... and with an option of the route broken as well: refused on the
        // option, group_start and pairs unread
        Frame back_mode(entry, 10, {0, 20, 10});
        back_mode.a.mode = SVA_FUSE_MIN_COST;
        report("min_cost_and_group_start_goes_back", entry, back_mode.a);
        Frame back_nv(entry, 10, {0, 20, 10});
        back_nv.a.n_valid = back_nv.n_valid.get();
        report("n_valid_and_group_start_goes_back", entry, back_nv.a);
        Frame back_unit(entry, 10, {0, 20, 10});
        back_unit.a.unit_baseline = back_unit.unit.get();
        report("unit_given_and_group_start_goes_back", entry, back_unit.a);
        Frame back_route(entry, 10, {0, 20, 10});
        back_route.a.route = array_route_of(3);
        report("unknown_route_and_group_start_goes_back", entry, back_route.a);
        Frame big(entry, 34, {0, 33, 34});
        report("group_of_33", entry, big.a);
        Frame full(entry, 33, {0, 32, 33});
        report("group_of_32", entry, full.a);
    }
    // the route numbers of the entry
    std::printf("routes|0|%d|\n", array_route_of(SVA_ARRAY_PAIRS) == ArrayRoute::Pairs &&
                                      array_route_of(SVA_ARRAY_GROUPS) == ArrayRoute::Groups &&
                                      array_route_of(SVA_ARRAY_GROUPS_MIXED) ==
                                          ArrayRoute::GroupsMixed &&
                                      array_route_of(3) == ArrayRoute::Unknown);
    // a default-built ArrayArgs is an old entry's: the new fields are off
    ArrayArgs d;
    std::printf("defaults|0|%d|\n", !d.sub && !d.subpix && d.route == ArrayRoute::Pairs);
    return 0;
}
"""


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """{(case, entry): (status, message)} as the program printed them; the
    sanitizers abort the program on any finding."""
    d = tmp_path_factory.mktemp("arraysubargs")
    src = d / "arraysubargs.cpp"
    src.write_text(PROGRAM)
    exe = d / "arraysubargs"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-g", "-I", CSRC, "-I", INC, str(src), "-o",
                    str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    out = {}
    for line in run.stdout.splitlines():
        name, entry, status, msg = line.split("|", 3)
        out[(name, int(entry))] = (int(status), msg)
    return out


def test_route_numbers_and_defaults(answers):
    assert answers[("routes", 0)] == (1, "")
    assert answers[("defaults", 0)] == (1, "")


@pytest.mark.parametrize("entry", OLD + SUB)
def test_valid_frames_pass(answers, entry):
    for case in ("valid", "group_of_32", "distance_fits", "no_subpix"):
        assert answers[(case, entry)] == (OK, ""), case


# ---- the old entries: every expectation of tests/test_array_args_cpu.py ------------
@pytest.mark.parametrize("case,routes,status,message", old.RULES,
                         ids=["%s-%s" % (r[0], "".join(map(str, r[1]))) for r in old.RULES])
def test_old_routes_refuse_as_before(answers, case, routes, status, message):
    for route in routes:
        assert answers[(case, route)] == (status, message), route


def test_old_routes_accept_as_before(answers):
    for case, routes in [("lr_check", old.PAIR), ("ref_differs", old.PAIR),
                         ("D_differs", old.PAIR), ("baseline_differs", old.PAIR + (MIXED,)),
                         ("null_unit", (DEPTH, CONF, MB)), ("mode", (DEPTH,)),
                         ("uniqueness_high", (DEPTH,)), ("distance", (DEPTH, CONF, MB))]:
        for route in routes:
            assert answers[(case, route)] == (OK, ""), (case, route)
    for route in OLD:
        assert answers[("group_start_goes_back", route)] == (UNSUPPORTED, "groups of 1..32 pairs")
        assert answers[("empty_group_and_bad_pair", route)] == (UNSUPPORTED,
                                                                "groups of 1..32 pairs")
    for route in old.PAIR:
        assert answers[("bad_pair_and_invalid_differs", route)] == (INVALID, "bad pair 3")
    for route in (CONF, MB, MIXED):
        assert answers[("uniqueness_and_null_images", route)] == (INVALID,
                                                                  "uniqueness must be 0..100")


def test_the_new_rules_are_no_rules_of_the_old_entries(answers):
    """What the old entries never set does not change what they answer: a plane
    or a unit baseline the new entry refuses is ignored there as before."""
    for route in (DEPTH, CONF, MB, MIXED):
        assert answers[("n_valid", route)] == (OK, ""), route
        assert answers[("unit_given", route)] == (OK, ""), route
    for route in (DEPTH, MB, MIXED):          # (sva_array_depth_conf takes both modes)
        assert answers[("min_cost", route)] == (OK, ""), route
    assert answers[("min_cost_planes", CONF)] == (OK, "")


# ---- the new entry ----------------------------------------------------------------
@pytest.mark.parametrize("case,routes,status,message", old.RULES,
                         ids=["%s-%s" % (r[0], "".join(map(str, r[1]))) for r in old.RULES])
def test_sub_routes_share_the_rules_of_their_old_entry(answers, case, routes, status, message):
    for entry in SUB:
        if LIKE[entry] in routes:
            assert answers[(case, entry)] == (status, message), entry


def test_sub_routes_accept_what_their_old_entry_accepts(answers):
    for case, entries in [("lr_check", (SUB_PAIRS,)), ("ref_differs", (SUB_PAIRS,)),
                          ("D_differs", (SUB_PAIRS,)),
                          ("baseline_differs", (SUB_PAIRS, SUB_MIXED)),
                          ("distance", (SUB_PAIRS, SUB_GROUPS)),
                          ("min_cost", (SUB_PAIRS,)), ("max_margin", (SUB_PAIRS,)),
                          ("min_cost_planes", (SUB_PAIRS,)), ("n_valid", (SUB_PAIRS,)),
                          ("unit_given", (SUB_MIXED,))]:
        for entry in entries:
            assert answers[(case, entry)] == (OK, ""), (case, entry)


@pytest.mark.parametrize("entry", OLD + SUB)
def test_unknown_route(answers, entry):
    for case in ("unknown_route", "negative_route", "unknown_route_and_null_group_start",
                 "unknown_route_and_group_start_goes_back"):
        assert answers[(case, entry)] == (INVALID, "unknown route"), case


def test_group_routes_take_the_median_only(answers):
    for entry in SUB_GROUP:
        for case in ("min_cost", "max_margin", "min_cost_planes", "min_cost_and_n_valid"):
            assert answers[(case, entry)] == (INVALID, GROUP_MODE), (case, entry)
        assert answers[("mode", entry)] == (INVALID, "unknown fusion mode")
        assert answers[("n_valid", entry)] == (INVALID, GROUP_PLANES)
        assert answers[("winner_median", entry)] == (INVALID, "the median has no winner map")
    for entry in SUB:
        assert answers[("mode", entry)] == (INVALID, "unknown fusion mode")
        assert answers[("winner_median", entry)] == (INVALID, "the median has no winner map")


def test_unit_baseline_belongs_to_the_mixed_route(answers):
    for entry in (SUB_PAIRS, SUB_GROUPS):
        assert answers[("unit_given", entry)] == (INVALID, UNIT_ELSEWHERE)
        assert answers[("null_unit", entry)] == (OK, "")
    assert answers[("null_unit", SUB_MIXED)] == (INVALID, "null unit_baseline")


def test_the_routes_options_come_first(answers):
    """Refused on the option although group_start goes back (pairs[10..19] do not
    exist: reading them would have ended the program) or another argument is bad."""
    for entry in SUB_GROUP:
        assert answers[("min_cost_and_group_start_goes_back", entry)] == (INVALID, GROUP_MODE)
        assert answers[("n_valid_and_group_start_goes_back", entry)] == (INVALID, GROUP_PLANES)
        assert answers[("n_valid_and_null_images", entry)] == (INVALID, GROUP_PLANES)
        assert answers[("uniqueness_and_min_cost", entry)] == (INVALID,
                                                               "uniqueness must be 0..100")
    for entry in (SUB_PAIRS, SUB_GROUPS):
        assert answers[("unit_given_and_group_start_goes_back", entry)] == (INVALID,
                                                                            UNIT_ELSEWHERE)
        assert answers[("unit_given_and_empty_group", entry)] == (INVALID, UNIT_ELSEWHERE)
    # with the options in order the sizes are what is refused, pairs still unread
    for entry in SUB:
        assert answers[("group_start_goes_back", entry)] == (UNSUPPORTED, "groups of 1..32 pairs")
        assert answers[("group_of_33", entry)] == (UNSUPPORTED, "groups of 1..32 pairs")
    assert answers[("min_cost_and_group_start_goes_back", SUB_PAIRS)] == (
        UNSUPPORTED, "groups of 1..32 pairs")
    assert answers[("n_valid_and_null_images", SUB_PAIRS)] == (INVALID, "bad array arguments")
