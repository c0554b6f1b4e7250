"""The rules of the four map filters (csrc/map_filter_args.h: check_cross,
check_speckle, check_fill, check_wmed) without a GPU: a host program with its
own main, built under AddressSanitizer and UBSan, reads a table of calls and
prints `status|message` for each.  The rule functions compare pointers and read
through none but view_step and guides, so the planes are fabricated addresses.

The expected status and message of a case are those of the refusal tables of
tests/test_cross_check_gpu.py, test_speckle_gpu.py, test_fill_gpu.py and
test_wmed_gpu.py where the case exists there, and otherwise those of the rules
as include/sva.h lists them.  Nothing is loaded into Python under a sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereovisionarray_amd", "csrc")
INC = os.path.join(ROOT, "include")
OK, INV, UNS = 0, 1, 2
INT_MAX, SIZE_MAX = 2 ** 31 - 1, 2 ** 64 - 1

PROGRAM = r"""
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "map_filter_args.h"
using namespace sva;
typedef unsigned long long u64;
template <class T> T* ptr(u64 v) { return reinterpret_cast<T*>((uintptr_t)v); }
// a line: filter disps subpix out out_sub n W H, then the filter's own arguments
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream f(argv[1]);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        char which;
        u64 d, s, o, os;
        long long n, W, H;
        in >> which >> d >> s >> o >> os >> n >> W >> H;
        const MapArgs m{ptr<const uint16_t>(d), ptr<const float>(s), (int)n, (int)W, (int)H, 0xFFFF,
                        ptr<uint16_t>(o), ptr<float>(os)};
        std::string msg;
        int st = -1;
        if (which == 'c') {
            long long md, ma, mc, ns;
            u64 ag, cf;
            in >> md >> ma >> mc >> ag >> cf >> ns;   // ns < 0: null view_step
            std::vector<int32_t> vs(ns > 0 ? 2 * ns : 2);
            for (long long i = 0; i < 2 * ns; i++) in >> vs[i];
            st = check_cross({m, ns < 0 ? nullptr : vs.data(), (int)md, (int)ma, (int)mc,
                              ptr<uint8_t>(ag), ptr<uint8_t>(cf)}, msg);
        } else if (which == 's') {
            long long ms, md;
            u64 size;
            in >> ms >> md >> size;
            st = check_speckle({m, (int)ms, (int)md, ptr<uint32_t>(size)}, msg);
        } else if (which == 'f') {
            long long md, mf, mode;
            u64 found;
            in >> md >> mf >> mode >> found;
            st = check_fill({m, (int)md, (int)mf, (int)mode, ptr<uint8_t>(found)}, msg);
        } else if (which == 'w') {
            long long r, ms, fill, ng;
            u64 pitch, w, sel, sup;
            in >> r >> ms >> fill >> pitch >> w >> sel >> sup >> ng;   // ng < 0: null guides
            std::vector<const uint8_t*> g(ng > 0 ? ng : 1);
            for (long long i = 0; i < ng; i++) {
                u64 a;
                in >> a;
                g[i] = ptr<const uint8_t>(a);
            }
            st = check_wmed({m, ng < 0 ? nullptr : g.data(), (size_t)pitch, ptr<const uint16_t>(w),
                             ptr<const uint8_t>(sel), (int)r, (int)ms, (int)fill, ptr<uint16_t>(sup)},
                            msg);
        }
        if (!in) return 3;
        std::printf("%d|%s\n", st, msg.c_str());
    }
    return 0;
}
"""

M_NULL, M_SIZE, M_SUB = "null pointer", "image size must be positive", "out_sub needs subpix"
M_N = {"c": "n_views must be 1..32", "s": "n_maps must be >= 1", "f": "n_maps must be >= 1",
       "w": "n_maps must be >= 1"}
M_BIG = {"c": "the cross-view check needs W * H < 2^31", "s": "the speckle filter needs W * H < 2^31",
         "f": "hole filling needs W * H < 2^31", "w": "the weighted median needs W * H < 2^31"}
M_IN_PLACE = ("an output overlaps an input or another output (in place: out == disps, "
              "out_sub == subpix)")
M_OVER = {"c": "an output overlaps an input", "s": M_IN_PLACE, "f": M_IN_PLACE,
          "w": "an output overlaps an input or another output (in place is not offered)"}

# n maps of W x H; every plane of a call in a region of its own, 2^40 apart
N, W, H = 2, 8, 4
B8 = N * W * H
REGION = {k: (i + 1) << 40 for i, k in enumerate(
    ["d", "s", "out", "osub", "agree", "conflict", "size", "found", "sel", "sup", "w", "g0", "g1"])}
STEPS = [(0, 0), (1, 0)]
# the bytes of a plane by its name (the guides: H rows of W, `pitch` apart, pitch = W + 3)
PITCH = W + 3
BYTES = dict(d=2 * B8, s=4 * B8, out=2 * B8, osub=4 * B8, agree=B8, conflict=B8, size=4 * B8,
             found=B8, sel=B8, sup=2 * B8, g0=(H - 1) * PITCH + W, g1=(H - 1) * PITCH + W)
# the filter's own planes, and which of them are outputs
OWN_OUT = {"c": [], "s": ["size"], "f": ["found"], "w": ["sup"]}
OWN_IN = {"c": [], "s": [], "f": [], "w": ["sel", "g0", "g1"]}


def call(which, **ch):
    """One line of the program's input: the good call of a filter with `ch` applied.
    A plane is None (null), a name (that plane's address) or (name, byte offset)."""
    a = dict(d="d", s="s", out="out", osub="osub", n=N, W=W, H=H, agree="agree",
             conflict="conflict", size="size", found="found", sel="sel", sup="sup", w="w",
             g=["g0", "g1"], pitch=PITCH, steps=STEPS, md=1, ma=1, mc=0, ms=20, mf=1, mode=1, r=2,
             sup_min=1, fill=1)
    a.update(ch)

    def at(v):
        if v is None:
            return 0
        if isinstance(v, int):
            return v
        name, off = (v, 0) if isinstance(v, str) else v
        return REGION[name] + off
    head = [which, at(a["d"]), at(a["s"]), at(a["out"]), at(a["osub"]), a["n"], a["W"], a["H"]]
    if which == "c":
        steps = a["steps"]
        own = [a["md"], a["ma"], a["mc"], at(a["agree"]), at(a["conflict"]),
               -1 if steps is None else len(steps)] + [v for st in steps or [] for v in st]
    elif which == "s":
        own = [a["ms"], a["md"], at(a["size"])]
    elif which == "f":
        own = [a["md"], a["mf"], a["mode"], at(a["found"])]
    else:
        g = a["g"]
        own = [a["r"], a["sup_min"], a["fill"], a["pitch"], at(a["w"]), at(a["sel"]), at(a["sup"]),
               -1 if g is None else len(g)] + [at(v) for v in g or []]
    return " ".join(str(v) for v in head + own)


def cases():
    """(name, line, status, message)."""
    out = []

    def add(name, which, status, msg, **ch):
        out.append((which + ":" + name, call(which, **ch), status, msg))
    own_bad = {   # a broken threshold of the filter's own, for the order cases
        "c": dict(md=-1), "s": dict(ms=-1), "f": dict(md=256), "w": dict(r=16)}
    own_msg = {"c": "max_diff must be >= 0", "s": "speckle max_size must be >= 0",
               "f": "fill max_dist must be 0..255", "w": "wmed radius must be 1..15"}
    for k in "csfw":
        add("good", k, OK, "")
        add("good_bare", k, OK, "", s=None, osub=None, agree=None, conflict=None, size=None,
            found=None, sel=None, sup=None, g=None, w=None)
        add("subpix_without_out_sub", k, OK, "", osub=None)
        # ---- every shared rule alone ----
        add("null_disps", k, INV, M_NULL, d=None)
        add("null_out", k, INV, M_NULL, out=None)
        add("n_0", k, INV, M_N[k], n=0)
        add("n_negative", k, INV, M_N[k], n=-1)
        add("zero_width", k, INV, M_SIZE, W=0)
        add("negative_height", k, INV, M_SIZE, H=-1)
        add("too_many_pixels", k, UNS, M_BIG[k], W=65536, H=32768)
        add("out_sub_without_subpix", k, INV, M_SUB, s=None)
        # ---- the order: each breaks the rule named first and later ones too ----
        add("null_before_n", k, INV, M_NULL, d=None, n=0, W=0, **own_bad[k])
        add("n_before_size", k, INV, M_N[k], n=0, H=0)
        add("size_before_unsupported", k, INV, M_SIZE, W=-1, H=INT_MAX, **own_bad[k])
        add("unsupported_before_own", k, UNS, M_BIG[k], W=65536, H=32768, **own_bad[k])
        add("own_before_out_sub", k, INV, own_msg[k], s=None, **own_bad[k])
        add("out_sub_before_overlap", k, INV, M_SUB, s=None, out=("d", 2))
        # ---- the exact aliases: in place for speckle and fill only ----
        in_place = (OK, "") if k in "sf" else (INV, M_OVER[k])
        add("out_is_disps", k, *in_place, out="d")
        add("out_sub_is_subpix", k, *in_place, osub="s")
        add("both_in_place", k, *in_place, out="d", osub="s")
        add("out_is_subpix", k, INV, M_OVER[k], out="s")
        add("out_sub_is_disps", k, INV, M_OVER[k], osub="d")
        # ---- every tested pair: output o laid over plane q ----
        outs = ["out", "osub"] + OWN_OUT[k]
        ins = ["d", "s"] + OWN_IN[k]
        pairs = [(o, q) for o in outs for q in ins]
        if k != "c":
            pairs += [(o, q) for i, o in enumerate(outs) for q in outs[i + 1:]]
        for o, q in pairs:
            bo, bq = BYTES[o], BYTES[q]
            for where, off, bad in (("inside", 2, True), ("last_byte", bq - 1, True),
                                    ("one_past", bq, False), ("first_byte", -(bo - 1), True),
                                    ("one_before", -bo, False)):
                add("%s_over_%s_%s" % (o, q, where), k, *((INV, M_OVER[k]) if bad else (OK, "")),
                    **{o: (q, off)})
    # ---- the cross-view check's own rules, and the pairs it does not test ----
    add("null_view_step", "c", INV, M_NULL, steps=None)
    add("n_33", "c", INV, M_N["c"], n=33)
    add("n_int_max", "c", INV, M_N["c"], n=INT_MAX, W=INT_MAX, H=1)
    add("step_256", "c", INV, "view_step components must be -255..255", steps=[(0, 0), (256, 0)])
    add("step_minus_256", "c", INV, "view_step components must be -255..255",
        steps=[(0, 0), (0, -256)])
    add("equal_steps", "c", INV, "two views have the same view_step", steps=[(3, 1), (3, 1)])
    add("max_diff_negative", "c", INV, "max_diff must be >= 0", md=-1)
    add("min_agree_32", "c", INV, "min_agree must be 0..31", ma=32)
    add("min_agree_negative", "c", INV, "min_agree must be 0..31", ma=-1)
    add("max_conflict_32", "c", INV, "max_conflict must be 0..31", mc=32)
    add("max_conflict_negative", "c", INV, "max_conflict must be 0..31", mc=-1)
    add("range_before_distinct", "c", INV, "view_step components must be -255..255",
        steps=[(256, 0), (256, 0)], md=-1)
    add("distinct_before_thresholds", "c", INV, "two views have the same view_step",
        steps=[(1, 1), (1, 1)], md=-1)
    add("max_diff_before_min_agree", "c", INV, "max_diff must be >= 0", md=-1, ma=32, mc=32)
    add("min_agree_before_max_conflict", "c", INV, "min_agree must be 0..31", ma=32, mc=32)
    for name, ch in (("out_over_out_sub", dict(out=("osub", 2))), ("agree_is_disps", dict(agree="d")),
                     ("agree_is_out", dict(agree="out")), ("conflict_in_subpix", dict(conflict=("s", 4))),
                     ("conflict_in_out_sub", dict(conflict=("osub", 8))),
                     ("agree_is_conflict", dict(conflict="agree"))):
        add("untested_" + name, "c", OK, "", **ch)
    # ---- the other filters' own rules ----
    add("max_size_negative", "s", INV, "speckle max_size must be >= 0", ms=-1)
    add("max_diff_negative", "s", INV, "speckle max_diff must be >= 0", md=-1)
    add("max_size_before_max_diff", "s", INV, "speckle max_size must be >= 0", ms=-1, md=-1)
    add("max_dist_negative", "f", INV, "fill max_dist must be 0..255", md=-1)
    add("max_dist_256", "f", INV, "fill max_dist must be 0..255", md=256)
    add("min_found_0", "f", INV, "fill min_found must be 1..8", mf=0)
    add("min_found_9", "f", INV, "fill min_found must be 1..8", mf=9)
    add("mode_negative", "f", INV, "fill mode must be 0..2", mode=-1)
    add("mode_3", "f", INV, "fill mode must be 0..2", mode=3)
    add("max_dist_before_min_found", "f", INV, "fill max_dist must be 0..255", md=256, mf=0, mode=3)
    add("min_found_before_mode", "f", INV, "fill min_found must be 1..8", mf=9, mode=3)
    add("radius_0", "w", INV, "wmed radius must be 1..15", r=0)
    add("radius_16", "w", INV, "wmed radius must be 1..15", r=16)
    add("min_support_0", "w", INV, "wmed min_support must be 1..961", sup_min=0)
    add("min_support_962", "w", INV, "wmed min_support must be 1..961", sup_min=962)
    add("fill_negative", "w", INV, "wmed fill must be 0 or 1", fill=-1)
    add("fill_2", "w", INV, "wmed fill must be 0 or 1", fill=2)
    add("guides_without_weights", "w", INV, "guides and weights go together", w=None)
    add("weights_without_guides", "w", INV, "guides and weights go together", g=None)
    add("null_guide", "w", INV, "null guide image", g=["g0", None])
    add("pitch_below_width", "w", INV, "guide pitch < width", pitch=W - 1)
    add("pitch_is_width", "w", OK, "", pitch=W)
    add("radius_before_min_support", "w", INV, "wmed radius must be 1..15", r=16, sup_min=0, fill=2)
    add("min_support_before_fill", "w", INV, "wmed min_support must be 1..961", sup_min=962,
        fill=2, w=None)
    add("fill_before_guides", "w", INV, "wmed fill must be 0 or 1", fill=2, w=None)
    add("pairing_before_null_guide", "w", INV, "guides and weights go together", w=None,
        g=[None, None])
    add("null_guide_before_pitch", "w", INV, "null guide image", g=[None, "g1"], pitch=1)
    add("pitch_before_out_sub", "w", INV, "guide pitch < width", pitch=0, s=None)
    # ---- byte counts that do not fit: a status, no overflow ----
    # n * W * H = (2^31 - 1)^2 < 2^62: the u8 count is exact, four times it still fits
    huge = dict(n=INT_MAX, W=INT_MAX, H=1, s=None, osub=None, size=None, found=None, sel=None,
                sup=None, g=None, w=None)
    b16 = 2 * INT_MAX * INT_MAX
    for k in "sfw":
        add("huge_apart", k, INV, M_OVER[k], **huge)     # 2^40 apart is inside 2^63 bytes
        add("huge_last_byte", k, INV, M_OVER[k], **dict(huge, d=4096, out=4096 + b16 - 1))
        add("huge_one_past", k, OK, "", **dict(huge, d=4096, out=4096 + b16))
    add("huge_in_place", "s", OK, "", **dict(huge, out="d"))
    add("huge_in_place", "f", OK, "", **dict(huge, out="d"))
    add("huge_in_place", "w", INV, M_OVER["w"], **dict(huge, out="d"))
    add("huge_32_views", "c", OK, "", n=32, W=INT_MAX, H=1, steps=[(i, 0) for i in range(32)],
        d=4096, s=None, osub=None, out=4096 + 64 * INT_MAX)
    add("huge_32_views_last_byte", "c", INV, M_OVER["c"], n=32, W=INT_MAX, H=1,
        steps=[(i, 0) for i in range(32)], d=4096, s=None, osub=None, out=4096 + 64 * INT_MAX - 1)
    # a guide's bytes (H - 1) * pitch + W: exact up to SIZE_MAX / 4, that count beyond
    cap = SIZE_MAX // 4
    fits = (cap - W) // (H - 1)
    lone = dict(s=None, osub=None, sup=None, sel=None, d=256, g=[1 << 20, 1 << 20])
    for name, pitch, size in (("pitch_fits", fits, (H - 1) * fits + W), ("pitch_saturates", fits + 1, cap),
                              ("pitch_near_size_max_over_h", SIZE_MAX // H, cap),
                              ("pitch_size_max", SIZE_MAX, cap)):
        add(name + "_last_byte", "w", INV, M_OVER["w"], **dict(lone, pitch=pitch, out=(1 << 20) + size - 1))
        add(name + "_one_past", "w", OK, "", **dict(lone, pitch=pitch, out=(1 << 20) + size))
    return out


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    d = tmp_path_factory.mktemp("map_filter_args")
    src, exe, table = d / "rules.cpp", d / "rules", d / "cases.txt"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-g", "-I", CSRC, "-I", INC, str(src), "-o",
                    str(exe)], check=True)
    table.write_text("".join(line + "\n" for _, line, _, _ in cases()))
    run = subprocess.run([str(exe), str(table)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases())
    return {name: tuple(line.split("|", 1)) for (name, _, _, _), line in zip(cases(), lines)}


def test_case_names_are_distinct():
    names = [c[0] for c in cases()]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("which", "csfw")
def test_rules(answers, which):
    mine = [c for c in cases() if c[0].startswith(which + ":")]
    assert len(mine) > 60
    wrong = [(name, answers[name], (status, msg)) for name, _, status, msg in mine
             if answers[name] != (str(status), msg)]
    assert not wrong, wrong
