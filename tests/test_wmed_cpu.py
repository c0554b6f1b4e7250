"""The weighted median filter without a GPU.

1. tests/wmed_expect.py's numpy form against its plain-Python walk, and the
   worked examples of the rule.
2. csrc/wmedian_math.h through a host program with its own main, built under
   AddressSanitizer and UBSan and run directly: the per-pixel routine (candidate
   test, weight lookup, bisection, tie walk) over whole small maps staged the way
   the kernel stages them, every output, count and source equal to wmed_expect.
3. The quality table of DESIGN.md §2.5e on tests/wmed_scene.py and
   tests/cross_scene.py.
4. array_args.h: the device-view planning function for 1..4 devices and the
   rules sva_array_depth_smoothed adds to check_array_args.
Nothing is loaded into Python under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

import cross_scene as cs
import fill_expect as fe
import speckle_expect as se
import wmed_expect as we
import wmed_scene as ws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereovisionarray_amd", "csrc")
INC = os.path.join(ROOT, "include")
INVALID = 0xFFFF
FLAT = np.ones(256, np.uint16)


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


def tables():
    """Named weight tables: an exponential, equal intensities only, the largest
    sums, nothing at all, and one that skips the centre itself."""
    only_equal = np.zeros(256, np.uint16)
    only_equal[0] = 3
    no_self = np.full(256, 5, np.uint16)
    no_self[0] = 0
    return {"sigma8": we.weights(8), "only_equal": only_equal,
            "largest": np.full(256, 65535, np.uint16), "zero": np.zeros(256, np.uint16),
            "no_self": no_self}


def random_guide(W, H, seed, levels=256):
    return np.random.default_rng(seed).integers(0, levels, (H, W)).astype(np.uint8)


# ---- the expectation itself --------------------------------------------------------
def test_weight_table():
    w = we.weights(32)
    assert w[0] == 1024 and w[32] == round(1024 / np.e) and w[255] == 0
    assert (np.diff(w.astype(int)) <= 0).all()
    assert we.weights(8)[56] == 1 and we.weights(8)[62] == 0


def test_numpy_form_equals_walk():
    """Holes at 0 %, 30 % and 100 %, radii up to wider than the frame, guided (by
    every table, the all-zero one included) and unguided, select, both fills."""
    rng = np.random.default_rng(11)
    tabs = list(tables().items())
    wrote = kept = zero_n = 0
    for trial in range(180):
        H, W = (int(v) for v in rng.integers(1, 13, 2))
        inv = (0xFFFF, 255, 0)[trial % 3]
        holes = (0.0, 0.3, 1.1)[trial // 3 % 3]
        d = fe.random_map(W, H, 2000 + trial, holes=holes, invalid=inv, hi=6)
        s = fe.subpix_of(d, trial)
        r = (1, 2, 5, 15)[trial // 9 % 4]
        name, tab = tabs[trial % len(tabs)]
        g = random_guide(W, H, trial, levels=(4, 256)[trial % 2]) if trial % 4 else None
        sel = (rng.random((H, W)) < 0.6).astype(np.uint8) if trial % 5 == 0 else None
        ms = (1, 2, 3, (2 * r + 1) ** 2, 961)[trial // 2 % 5]
        for fill in (0, 1):
            kw = dict(weights=None if g is None else tab, subpix=s, select=sel, min_support=ms,
                      fill=fill)
            out, osub, sup, written = we.weighted_median(d, inv, r, g, **kw)
            w_out, w_sub, w_sup, w_written = we.walk(d, inv, r, g, **kw)
            assert np.array_equal(out, w_out), (trial, fill)
            assert same32(osub, w_sub) and np.array_equal(sup, w_sup)
            assert np.array_equal(written, w_written)
            assert np.array_equal(out[~written], d[~written])
            assert same32(osub[~written], s[~written])
            if g is not None and name == "zero":
                assert not written.any() and not sup.any()
            wrote += int(written.sum())
            kept += int((~written).sum())
            zero_n += int(((sup == 0) & ~written).sum())
    assert wrote > 1000 and kept > 1000 and zero_n > 100


def test_flat_weights_are_the_sorted_window_lower_median():
    """On a fully valid map the unguided filter, and the guided one with flat
    weights, give element (n - 1) // 2 of the sorted window."""
    H, W, r = 9, 11, 2
    d = fe.random_map(W, H, 3, holes=0.0, hi=30)
    want = np.zeros_like(d)
    for y in range(H):
        for x in range(W):
            win = sorted(d[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1].ravel().tolist())
            want[y, x] = win[(len(win) - 1) // 2]
    out, _, sup, written = we.weighted_median(d, INVALID, r)
    assert np.array_equal(out, want) and written.all()
    assert sup[4, 5] == 25 and sup[0, 0] == 9
    flat = we.weighted_median(d, INVALID, r, random_guide(W, H, 1), FLAT)
    assert np.array_equal(flat[0], want) and np.array_equal(flat[2], sup)


def edge_maps(shift):
    """(d, g): a background 4 / foreground 10 step at x = 16 in the guide (0 |
    255: sigma 32 gives that difference the weight 0) and at x = 16 - shift in
    d: the foreground fattened by `shift`."""
    d = np.full((20, 32), 4, np.uint16)
    d[:, 16 - shift:] = 10
    g = np.zeros((20, 32), np.uint8)
    g[:, 16:] = 255
    return d, g


def test_a_step_edge_with_its_guide_stays_in_place():
    d, g = edge_maps(0)
    out, _, _, written = we.weighted_median(d, INVALID, 5, g, we.weights(32))
    assert written.all() and np.array_equal(out, d)


def test_a_fattened_edge_comes_back_to_the_guide_edge():
    """The foreground reaches 3 px into the background; with the true guide the
    filter at r = 5 puts the edge back, and the unguided median leaves it.  Three
    is the most r = 5 undoes: the last background column sees three fattened
    columns against three true ones, and the LOWER median takes the background."""
    truth, g = edge_maps(0)
    d, _ = edge_maps(3)
    assert (d != truth).sum() == 3 * 20
    out = we.weighted_median(d, INVALID, 5, g, we.weights(32))[0]
    assert np.array_equal(out, truth)
    plain = we.weighted_median(d, INVALID, 5)[0]
    assert np.array_equal(plain, d)


# ---- wmedian_math.h ----------------------------------------------------------------
MATH_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "wmedian_math.h"
using namespace sva;

#define REQUIRE(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)

// the staged planes of one map: the frame and an r-wide halo, as the kernel's LDS tile
struct Window {
    const std::vector<uint16_t>* sd;
    const std::vector<uint8_t>* sg;
    const std::vector<uint16_t>* tab;
    int stride, rows, x, y, r;   // (x, y): the window's top-left cell
    size_t at(int i, int j) const {
        if (i < 0 || i > 2 * r || j < 0 || j > 2 * r) std::abort();    // outside the window
        if (x + i >= stride || y + j >= rows) std::abort();            // outside the staging
        return (size_t)(y + j) * stride + (x + i);
    }
    unsigned d(int i, int j) const { return (*sd)[at(i, j)]; }
    unsigned g(int i, int j) const { return (*sg)[at(i, j)]; }
    unsigned w(int delta) const {
        if (delta < 0 || delta > 255) std::abort();
        return (*tab)[delta];
    }
};

static int rules() {
    REQUIRE(!wm::thresholds_error(1, 1, 0) && !wm::thresholds_error(15, 961, 1));
    REQUIRE(wm::thresholds_error(0, 1, 0) && wm::thresholds_error(16, 1, 0));
    REQUIRE(wm::thresholds_error(1, 0, 0) && wm::thresholds_error(1, 962, 0));
    REQUIRE(wm::thresholds_error(1, 1, -1) && wm::thresholds_error(1, 1, 2));
    REQUIRE(wm::staged(0, 77) == 0 && wm::staged(77, 77) == 0 && wm::staged(65535, 77) == 65535);
    REQUIRE(wm::considered(1, 1, 0, 77) && !wm::considered(0, 1, 5, 77));
    REQUIRE(!wm::considered(1, 0, 77, 77) && wm::considered(9, 0, 5, 77));
    return 0;
}

// cases: W H invalid r min_support fill guided selected, then H * W values of d,
// (guided) H * W of g and 256 weights, (selected) H * W of select.  Per pixel:
// out, support, the source index (-1: not written).
static int cases(std::FILE* f) {
    int W, H, invalid, r, ms, fill, guided, selected;
    while (std::fscanf(f, "%d %d %d %d %d %d %d %d", &W, &H, &invalid, &r, &ms, &fill, &guided,
                       &selected) == 8) {
        const size_t np = (size_t)W * H;
        std::vector<unsigned> d(np), g(np, 0), sel(np, 1), tab(256, 0);
        for (unsigned& v : d) REQUIRE(std::fscanf(f, "%u", &v) == 1);
        if (guided) {
            for (unsigned& v : g) REQUIRE(std::fscanf(f, "%u", &v) == 1);
            for (unsigned& v : tab) REQUIRE(std::fscanf(f, "%u", &v) == 1);
        }
        if (selected)
            for (unsigned& v : sel) REQUIRE(std::fscanf(f, "%u", &v) == 1);
        REQUIRE(!wm::thresholds_error(r, ms, fill));
        const int sw = W + 2 * r, sh = H + 2 * r;
        std::vector<uint16_t> sd((size_t)sw * sh, 0), t16(tab.begin(), tab.end());
        std::vector<uint8_t> sg((size_t)sw * sh, 0);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                sd[(size_t)(y + r) * sw + x + r] = (uint16_t)wm::staged(d[(size_t)y * W + x], (unsigned)invalid);
                sg[(size_t)(y + r) * sw + x + r] = (uint8_t)g[(size_t)y * W + x];
            }
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const size_t p = (size_t)y * W + x;
                unsigned out = d[p], n = 0;
                long src = -1;
                if (wm::considered(sel[p], fill, d[p], (unsigned)invalid)) {
                    const Window win{&sd, &sg, &t16, sw, sh, x, y, r};
                    const wm::Pick k = guided ? wm::pick<true>(win, r, (int)g[p], ms)
                                              : wm::pick<false>(win, r, 0, ms);
                    n = k.n;
                    if (k.written) {
                        out = k.d;
                        src = (long)(y + k.j - r) * W + (x + k.i - r);
                        REQUIRE(y + k.j - r >= 0 && y + k.j - r < H && x + k.i - r >= 0 && x + k.i - r < W);
                    }
                }
                std::printf("%u %u %ld\n", out, n, src);
            }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 1) return rules();
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    const int s = cases(f);
    std::fclose(f);
    return s;
}
"""


@pytest.fixture(scope="module")
def math_exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("wmedmath"), "wmedmath", MATH_PROGRAM)


def test_rules_of_the_header(math_exe):
    run = subprocess.run([math_exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "" and run.stdout == "", run.stdout + run.stderr


def math_cases():
    """(W, H, invalid, r, min_support, fill, g, tab, sel, d)."""
    cases = []
    rng = np.random.default_rng(31)
    frames = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (8, 8), (11, 6), (12, 12), (33, 9)]
    tabs = list(tables().values())
    n = 0
    for W, H in frames:
        for r in (1, 2, 7, 15):
            for holes in (0.0, 0.3, 0.9, 1.1):
                inv = (0xFFFF, 77, 0)[n % 3]
                d = fe.random_map(W, H, 7000 + n, holes=holes, invalid=inv,
                                  hi=(5, 40, 60000)[n % 3])
                g = random_guide(W, H, n, levels=(3, 256)[n % 2]) if n % 3 else None
                tab = tabs[n % len(tabs)]
                sel = (rng.random((H, W)) < 0.5).astype(np.uint8) if n % 4 == 1 else None
                ms = (1, 2, (2 * r + 1) ** 2, 961, 4)[n % 5]
                cases.append((W, H, inv, r, ms, n // 2 % 2, g, tab, sel, d))
                n += 1
    return cases


def test_per_pixel_routine_equals_wmed_expect(math_exe, tmp_path):
    cases = math_cases()
    path = tmp_path / "cases.txt"
    line = lambda a: " ".join(str(int(v)) for v in np.asarray(a).ravel()) + "\n"
    with open(path, "w") as f:
        for W, H, inv, r, ms, fill, g, tab, sel, d in cases:
            f.write("%d %d %d %d %d %d %d %d\n" % (W, H, inv, r, ms, fill, g is not None,
                                                   sel is not None))
            f.write(line(d))
            if g is not None:
                f.write(line(g) + line(tab))
            if sel is not None:
                f.write(line(sel))
    run = subprocess.run([math_exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-400:] + run.stderr
    rows = np.array([[int(v) for v in ln.split()] for ln in run.stdout.splitlines()],
                    dtype=np.int64)
    assert rows.shape == (sum(c[0] * c[1] for c in cases), 3)
    at = written_seen = 0
    for W, H, inv, r, ms, fill, g, tab, sel, d in cases:
        got = rows[at:at + W * H]
        at += W * H
        s = np.arange(W * H, dtype=np.float32).reshape(H, W)     # subpix = the pixel's index
        out, osub, sup, written = we.weighted_median(
            d, inv, r, g, None if g is None else tab, s, sel, ms, fill)
        where = (W, H, r, ms, fill, g is not None)
        assert np.array_equal(got[:, 0].reshape(H, W), out), where
        assert np.array_equal(got[:, 1].reshape(H, W), sup), where
        src = got[:, 2].reshape(H, W)
        assert np.array_equal(src >= 0, written), where
        assert np.array_equal(src[written], osub[written].astype(np.int64)), where
        written_seen += int(written.sum())
    assert written_seen > 2000


# ---- the rule on the two scenes ----------------------------------------------------
def chain(scene):
    """(after check + speckle, after fill) of a scene, from the CPU expectations."""
    checked = scene.checked(**scene.CHECK)[0]
    filtered = se.filter_speckles(checked, scene.INVALID, 20, 1)[0]
    filled = fe.fill_holes(filtered, scene.INVALID, 16, 3, fe.MEDIAN)[0]
    return filtered, filled


def table_of(scene, guides):
    filtered, filled = chain(scene)
    truth = scene.views_and_truth()[1]
    q = lambda m: ws.quality(m, truth)
    guided = we.weighted_median(filled, scene.INVALID, 5, guides, we.weights(32))[0]
    same_r = we.weighted_median(filled, scene.INVALID, 5)[0]
    plain = we.weighted_median(filled, scene.INVALID, 1, fill=0)[0]
    return dict(filtered=q(filtered), filled=q(filled), guided=q(guided), unguided_r5=q(same_r),
                plain_r1=q(plain))


# stage: (wrong, correct, holes) over the interior of the nine maps, as
# wmed_expect produces them
BANDED = dict(filtered=(448, 64940, 2004), filled=(834, 66558, 0), guided=(359, 67033, 0),
              unguided_r5=(1083, 66309, 0), plain_r1=(786, 66606, 0))
CROSS = dict(filtered=(454, 65532, 1406), filled=(723, 66669, 0), guided=(1123, 66269, 0),
             unguided_r5=(1006, 66386, 0), plain_r1=(701, 66691, 0))


def test_quality_table_banded_scene():
    """The image knows where the surface ends: the guided filter leaves strictly
    fewer wrong pixels than the fill, and than the unguided filter of its radius."""
    t = table_of(ws, np.stack(ws.views()))
    print("banded", t)
    assert t["guided"][0] < t["filled"][0]
    assert t["guided"][0] < t["unguided_r5"][0]
    assert t["filled"][2] == 0 and t["guided"][2] == 0
    assert t == BANDED


def test_quality_table_cross_scene():
    """Both surfaces are full-range noise, the image carries no depth cue: the
    counts are pinned, and the documentation says the guide hurts here."""
    t = table_of(cs, np.stack(cs.views()))
    print("cross", t)
    assert t["filtered"] == (454, 65532, 1406)
    assert t == CROSS


# ---- array_args.h: view planning and the smoothed frame's rules ---------------------
PLAN_PROGRAM = r"""
#include <cstdio>
#include <set>
#include <vector>
#include "array_args.h"
using namespace sva;

#define REQUIRE(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
    // five groups of a 3x3 rig: camera r against some neighbours
    const int n_images = 9;
    const int refs[5] = {4, 0, 8, 2, 4};
    std::vector<sva_array_pair> pairs;
    std::vector<int> group_of;
    for (int g = 0; g < 5; g++)
        for (int o = g; o < 9; o += 3)
            if (o != refs[g]) {
                sva_array_pair p{};
                p.ref = refs[g];
                p.other = o;
                pairs.push_back(p);
                group_of.push_back(g);
            }
    const int n_pairs = (int)pairs.size();
    for (int nd = 1; nd <= 4; nd++)
        for (int on0 = 0; on0 < 2; on0++) {
            std::vector<int32_t> dev_of(n_pairs);
            for (int j = 0; j < n_pairs; j++) dev_of[j] = group_of[j] % nd;
            std::vector<std::vector<int>> slot;
            std::vector<int> n_need;
            std::vector<char> used;
            plan_views(nd, n_images, pairs.data(), n_pairs, dev_of.data(), on0 != 0, slot, n_need, used);
            REQUIRE((int)slot.size() == nd && (int)n_need.size() == nd && (int)used.size() == n_images);
            for (int d = 0; d < nd; d++) {
                // what the device must hold, stated directly
                std::set<int> want;
                for (int j = 0; j < n_pairs; j++) {
                    if (dev_of[j] == d) {
                        want.insert(pairs[j].ref);
                        want.insert(pairs[j].other);
                    }
                    if (on0 && d == 0) want.insert(pairs[j].ref);
                }
                std::set<int> slots;
                for (int v = 0; v < n_images; v++) {
                    REQUIRE((slot[d][v] >= 0) == (want.count(v) == 1));
                    if (slot[d][v] >= 0) {
                        REQUIRE(slot[d][v] < n_need[d] && slots.insert(slot[d][v]).second);
                        REQUIRE(used[v]);
                    }
                }
                REQUIRE((int)slots.size() == n_need[d] && n_need[d] == (int)want.size());
            }
            // without the flag the plan is the one the frames always had, and with it
            // only device 0 gains views, behind the slots it already had
            if (on0) {
                std::vector<std::vector<int>> base;
                std::vector<int> base_need;
                std::vector<char> base_used;
                plan_views(nd, n_images, pairs.data(), n_pairs, dev_of.data(), false, base, base_need, base_used);
                for (int d = 1; d < nd; d++) REQUIRE(slot[d] == base[d]);
                for (int v = 0; v < n_images; v++)
                    REQUIRE(base[0][v] < 0 ? slot[0][v] < 0 || slot[0][v] >= base_need[0]
                                           : slot[0][v] == base[0][v]);
                std::printf("%d %d\n", nd, n_need[0] - base_need[0]);
            }
        }
    return 0;
}
"""


def test_view_planning_for_one_to_four_devices(tmp_path):
    exe = build(tmp_path, "wmedplan", PLAN_PROGRAM)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    extra = dict(tuple(int(v) for v in ln.split()) for ln in run.stdout.splitlines())
    # one device holds everything already; with more, device 0 gains the
    # reference views of the groups that run elsewhere
    assert extra[1] == 0 and set(extra) == {1, 2, 3, 4} and all(extra[n] >= 0 for n in extra)
    # worked by hand for this rig: device 0 lacks camera 8 with three devices,
    # cameras 8 and 2 with four
    assert extra == {1: 0, 2: 0, 3: 1, 4: 2}


SMOOTH_ARGS_PROGRAM = r"""
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
    // {fill_mode, wmed_radius, wmed_min_support, wmed_select}
    const int rows[][4] = {{0, 1, 1, 0},  {2, 15, 961, 1}, {0, 0, 1, 0},   {0, 16, 1, 0},
                           {0, 5, 0, 0},  {0, 5, 962, 0},  {0, 5, 1, -1},  {0, 5, 1, 2},
                           {0, 16, 0, 2}, {0, 5, 962, 2},  {3, 16, 1, 0}};
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
        a.fill = true;
        a.fill_max_dist = 4;
        a.fill_min_found = 1;
        a.fill_mode = r[0];
        a.wmed = true;
        a.wmed_radius = r[1];
        a.wmed_min_support = r[2];
        a.wmed_select = r[3];
        std::string msg;
        std::vector<int32_t> ratio;
        const int st = check_array_args(a, msg, ratio);
        std::printf("%d|%s\n", st, msg.c_str());
        // without a.wmed the filter's values are not looked at
        a.wmed = false;
        const int st0 = check_array_args(a, msg, ratio);
        if (r[0] <= 2 && st0 != SVA_OK) return 1;
    }
    return 0;
}
"""


def test_smoothed_entry_rules(tmp_path):
    exe = build(tmp_path, "wmedargs", SMOOTH_ARGS_PROGRAM)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    got = [tuple(line.split("|")) for line in run.stdout.splitlines()]
    rad, sup, sel = ("wmed radius must be 1..15", "wmed min_support must be 1..961",
                     "wmed select must be 0 or 1")
    want = [("0", ""), ("0", ""), ("1", rad), ("1", rad), ("1", sup), ("1", sup), ("1", sel),
            ("1", sel), ("1", rad), ("1", sup), ("1", "fill mode must be 0..2")]
    assert got == want
