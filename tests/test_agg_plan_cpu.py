"""The aggregation plan (csrc/agg_plan.h) without a GPU.  The
header -- plain C++, the one sva_api.cpp and the two launchers compile -- is
built into a host program under AddressSanitizer and UBSan that prints every
plan of the shapes below; the sizes, routes and offsets expected here are
restated from DESIGN.md (checkpoints every `seg` pixels: hck = 2*H*ceil(W/seg)*D,
vck = 2*ceil(H/seg)*W*D, eight minima bytes per segment) and from the tuning
constants the program prints, not from the header's functions."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereovisionarray_amd", "csrc")
INC = os.path.join(ROOT, "include")

SHAPES = [(1, 1), (3, 40), (40, 3), (16, 8), (15, 9), (65, 31), (333, 77), (1920, 1080),
          (3840, 2160)]
NATIVE = (64, 128, 192, 256)
P2S = (0, 127, 128, 193)
BATCHES = (1, 3, 4, 8)
EIGHT, FOUR, PAIR = 0, 1, 2

PROGRAM = r"""
#include <cstdio>
#include "agg_plan.h"
using namespace sva;

const int kShapes[][2] = {{1, 1}, {3, 40}, {40, 3}, {16, 8}, {15, 9}, {65, 31}, {333, 77},
                          {1920, 1080}, {3840, 2160}};
const int kD[] = {64, 128, 192, 256}, kP2[] = {0, 127, 128, 193}, kBatch[] = {1, 3, 4, 8};

// kind|key|valid|every field of the plan|carve's offsets (-1: a null pointer)
void dump(const char* kind, long long key, const AggPlan& p) {
    uint8_t* const paths = (uint8_t*)((uintptr_t)1 << 40);
    uint8_t* const ckpt = (uint8_t*)((uintptr_t)1 << 41);
    const AggBuffers b = carve(p, nullptr, paths, ckpt);
    auto off = [](const uint8_t* q, const uint8_t* base) { return q ? (long long)(q - base) : -1ll; };
    std::printf("%s|%lld|%d|%d %d %d %d %d %d %d %d %d %d|%d %d %d %d %zu %zu %zu %zu|%zu %zu %zu|"
                "%zu %zu %zu %zu|%zu %zu %zu %zu|%lld %lld %lld %lld|%d\n",
                kind, key, (int)plan_valid(p), p.W, p.H, p.D, p.dreal, p.P1, p.P2, p.dmin, p.frames,
                (int)p.route, (int)p.minima, p.tg.seg_log2, p.tg.ntx, p.tg.nty, p.tg.nsx,
                p.tg.hck_bytes, p.tg.vck_bytes, p.tg.hmn_bytes, p.tg.vmn_bytes, p.vol, p.paths_bytes,
                p.ckpt_bytes, p.hck_off, p.vck_off, p.pair_off, p.mn_off, p.c_stride, p.vol_stride,
                p.hck_stride, p.vck_stride, off(b.volumes, paths), off(b.CK, ckpt), off(b.CKV, ckpt),
                off(b.MN, ckpt), (int)buffers_fit(p, b));
}

int main() {
    std::printf("tune|%d %d %d %d|%d %d %d %d|%d %d|%lld\n", tune::kDiagPair4, tune::kDiagPair8,
                tune::kDiagPair12, tune::kDiagPair16, tune::kPathMinima4, tune::kPathMinima8,
                tune::kPathMinima12, tune::kPathMinima16, tune::kWtahvTileLog2,
                tune::kWtahvTileLog2Wide, tune::kDiagPairMinPixels);
    for (auto& wh : kShapes)
        for (int D : kD) {
            const int W = wh[0], H = wh[1];
            const long long thr[] = {0, (long long)W * H, (long long)W * H + 1, tune::kDiagPairMinPixels};
            for (int dreal : {D, D - 28}) {
                for (int P2 : kP2)
                    for (long long t : thr) dump("frame", t, frame_plan(AggShape{W, H, D, dreal, 7, P2, 5}, t));
                for (int m : kBatch) dump("batch", m, batch_plan(AggShape{W, H, D, dreal, 10, 120, 5}, m));
                dump("stage", 0, stage_plan(AggShape{W, H, D, dreal, 10, 120, 5}));
                dump("eight", 0, eight_plan(AggShape{W, H, D, dreal, 10, 120, 5}));
            }
            const AggReserve r = reserve_plan(W, H, D);
            std::printf("reserve|%d %d %d|%zu %zu\n", W, H, D, r.paths_bytes, r.ckpt_bytes);
        }
    // a D with no native class reserves like a class without pair route and minima
    for (int D : {100, 320}) {
        const AggReserve r = reserve_plan(65, 31, D);
        std::printf("reserve|%d %d %d|%zu %zu\n", 65, 31, D, r.paths_bytes, r.ckpt_bytes);
    }
    // refusals, at the class that has both the pair route and minima (if any does)
    const AggShape s{65, 31, 128, 128, 10, 120, 0};
    dump("ok_pair", 0, agg_plan(s, 1, AggRoute::Pair, false));
    dump("ok_minima", 0, agg_plan(s, 1, AggRoute::Four, true));
    dump("bad_pair_batch", 0, agg_plan(s, 3, AggRoute::Pair, false));
    dump("bad_minima_batch", 0, agg_plan(s, 3, AggRoute::Four, true));
    dump("bad_minima_eight", 0, agg_plan(s, 1, AggRoute::Eight, true));
    dump("bad_eight_batch", 0, agg_plan(s, 2, AggRoute::Eight, false));
    dump("bad_pair_p2", 0, agg_plan(AggShape{65, 31, 128, 128, 10, 128, 0}, 1, AggRoute::Pair, false));
    dump("bad_pair_class", 0, agg_plan(AggShape{65, 31, 64, 64, 10, 120, 0}, 1, AggRoute::Pair, false));
    dump("bad_minima_class", 0, agg_plan(AggShape{65, 31, 64, 64, 10, 120, 0}, 1, AggRoute::Four, true));
    dump("bad_no_frames", 0, batch_plan(s, 0));
    dump("ok_below_4g", 0, stage_plan(AggShape{65536, 1023, 64}));
    dump("bad_4g", 0, stage_plan(AggShape{65536, 1024, 64}));
    dump("bad_4g_frame", 0, frame_plan(AggShape{65536, 512, 128, 128, 10, 120, 0}, 0));
    dump("bad_4g_eight", 0, eight_plan(AggShape{32768, 512, 256}));
    dump("bad_d_100", 0, frame_plan(AggShape{65, 31, 100, 100, 10, 120, 0}, 0));
    dump("bad_d_320", 0, stage_plan(AggShape{65, 31, 320}));
    dump("bad_d_0", 0, eight_plan(AggShape{65, 31, 0}));
    // buffers that do not fit their plan
    {
        uint8_t x = 0;
        const AggPlan f = frame_plan(s, 0), e = eight_plan(s), st = stage_plan(s);
        std::printf("fit|%d %d %d %d %d %d\n", (int)buffers_fit(st, AggBuffers{&x, &x, &x, &x, nullptr}),
                    (int)buffers_fit(st, AggBuffers{&x, &x, &x, nullptr, nullptr}),
                    (int)buffers_fit(st, AggBuffers{&x, &x, nullptr, &x, nullptr}),
                    (int)buffers_fit(e, AggBuffers{&x, &x, &x, &x, nullptr}),
                    (int)buffers_fit(e, AggBuffers{&x, &x, nullptr, nullptr, nullptr}),
                    (int)buffers_fit(f, AggBuffers{&x, &x, &x, &x, nullptr}) == !f.minima);
    }
    return 0;
}
"""

FIELDS = ("W H D dreal P1 P2 dmin frames route minima|seg_log2 ntx nty nsx hck vck hmn vmn|"
          "vol paths_bytes ckpt_bytes|hck_off vck_off pair_off mn_off|"
          "c_stride vol_stride hck_stride vck_stride|b_volumes b_ck b_ckv b_mn|fits")


class Plan:
    def __init__(self, kind, key, valid, groups):
        self.kind, self.key, self.valid = kind, int(key), bool(int(valid))
        for names, values in zip(FIELDS.split("|"), groups):
            for n, v in zip(names.split(), values.split()):
                setattr(self, n, int(v))


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    """What the program printed: the plans by kind, the tuning constants, the
    reserve sizes.  The sanitizers abort the program on any finding."""
    d = tmp_path_factory.mktemp("aggplan")
    src = d / "aggplan.cpp"
    src.write_text(PROGRAM)
    exe = d / "aggplan"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-g", "-I", CSRC, "-I", INC, str(src), "-o",
                    str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr

    class Out:
        plans, reserve = {}, {}
    o = Out()
    for line in run.stdout.splitlines():
        f = line.split("|")
        if f[0] == "tune":
            pair, mn, log2, thr = ([int(v) for v in g.split()] for g in f[1:])
            o.pair = dict(zip(NATIVE, (bool(v) for v in pair)))
            o.minima = dict(zip(NATIVE, (bool(v) for v in mn)))
            o.seg = {D: 1 << log2[0 if D <= 128 else 1] for D in NATIVE}
            o.default_threshold = thr[0]
        elif f[0] == "reserve":
            o.reserve[tuple(int(v) for v in f[1].split())] = tuple(int(v) for v in f[2].split())
        elif f[0] == "fit":
            o.fit = [int(v) for v in f[1].split()]
        else:
            o.plans.setdefault(f[0], []).append(Plan(f[0], f[1], f[2], f[3:]))
    return o


def ceil_div(a, b):
    return -(-a // b)


def sizes(o, W, H, D):
    """DESIGN.md's plane sizes, restated: (vol, hck, vck, hmn, vmn)."""
    seg = o.seg.get(D, 8)
    nsx, nsy = ceil_div(W, seg), ceil_div(H, seg)
    return W * H * D, 2 * H * nsx * D, 2 * nsy * W * D, 2 * H * nsx * 8, 2 * nsy * W * 8


def every_plan(o):
    return [p for k in ("frame", "batch", "stage", "eight") for p in o.plans[k]]


def test_every_case_was_planned(out):
    n = len(SHAPES) * len(NATIVE) * 2
    assert len(out.plans["frame"]) == n * len(P2S) * 4
    assert len(out.plans["batch"]) == n * len(BATCHES)
    assert len(out.plans["stage"]) == n and len(out.plans["eight"]) == n
    seen = {(p.W, p.H, p.D, p.dreal) for p in every_plan(out)}
    assert seen == {(W, H, D, dr) for (W, H), D in itertools.product(SHAPES, NATIVE)
                    for dr in (D, D - 28)}
    assert all(p.valid and p.fits for p in every_plan(out))


def test_sizes_equal_the_restated_formulas(out):
    for p in every_plan(out):
        vol, hck, vck, hmn, vmn = sizes(out, p.W, p.H, p.D)
        seg = out.seg[p.D]
        assert (1 << p.seg_log2, p.ntx, p.nty, p.nsx) == (
            seg, ceil_div(p.W, 16), ceil_div(p.H, seg), ceil_div(p.W, seg)), vars(p)
        assert (p.vol, p.hck, p.vck, p.hmn, p.vmn) == (vol, hck, vck, hmn, vmn), vars(p)
        nvol = {EIGHT: 8, FOUR: 4, PAIR: 2}[p.route]
        assert p.paths_bytes == nvol * vol * p.frames, vars(p)
        ck = 0 if p.route == EIGHT else (hck + vck) * p.frames
        ck += vck if p.route == PAIR else 0            # one row-checkpoint plane per diagonal pair
        ck += hmn + vmn if p.minima else 0
        assert p.ckpt_bytes == ck, vars(p)
        assert (p.P1, p.dmin) == ((7, 5) if p.kind == "frame" else (10, 5))


# sva_tile_layout_of of the parent commit: (seg, nsx, nsy, diag_volumes,
# cost_bytes, diag_bytes, hckpt_bytes, vckpt_bytes)
PARENT_LAYOUT = {
    (65, 31, 128): (8, 9, 4, 4, 257920, 1031680, 71424, 66560),
    (333, 77, 192): (8, 42, 10, 4, 4923072, 19692288, 1241856, 1278720),
    (1920, 1080, 128): (8, 240, 135, 4, 265420800, 1061683200, 66355200, 66355200),
}


def test_stage_plan_is_the_tile_layout(out):
    """The stage plan carries what sva_tile_layout_of returns (sva_api.cpp
    tile_layout copies these fields): the restated layout for every shape, the
    parent's recorded values for three (recorded at 8-pixel tiles)."""
    got = {}
    for p in out.plans["stage"]:
        vol, hck, vck, _, _ = sizes(out, p.W, p.H, p.D)
        seg = out.seg[p.D]
        layout = (1 << p.seg_log2, p.nsx, p.nty, 4, p.vol, p.paths_bytes, p.hck, p.vck)
        assert layout == (seg, ceil_div(p.W, seg), ceil_div(p.H, seg), 4, vol, 4 * vol, hck, vck)
        assert (p.route, p.frames, p.minima) == (FOUR, 1, 0)
        got[(p.W, p.H, p.D)] = layout
    for shape, layout in PARENT_LAYOUT.items():
        if out.seg[shape[2]] == 8:
            assert got[shape] == layout, shape


def test_frame_route(out):
    """Pair exactly when the D class has it, 2 * P2 fits a u8 and the frame has
    the threshold's pixels; minima exactly when the class has them."""
    thresholds = set()
    for p in out.plans["frame"]:
        pair = out.pair[p.D] and 2 * p.P2 <= 255 and p.W * p.H >= p.key
        assert p.route == (PAIR if pair else FOUR), vars(p)
        assert p.minima == out.minima[p.D] and p.frames == 1, vars(p)
        assert p.dreal in (p.D, p.D - 28)
        thresholds.add((p.W, p.H, p.key))
    for W, H in SHAPES:
        for t in (0, W * H, W * H + 1, out.default_threshold):
            assert (W, H, t) in thresholds
    assert {p.P2 for p in out.plans["frame"]} == set(P2S)
    if any(out.pair.values()):      # both routes were seen
        assert {p.route for p in out.plans["frame"]} == {FOUR, PAIR}


def test_other_plans_route(out):
    for p in out.plans["batch"] + out.plans["stage"]:
        assert (p.route, p.minima) == (FOUR, 0), vars(p)
    for p in out.plans["eight"]:
        assert (p.route, p.minima, p.frames) == (EIGHT, 0, 1), vars(p)
    assert sorted({p.frames for p in out.plans["batch"]}) == list(BATCHES)
    assert all(p.frames == p.key for p in out.plans["batch"])


def test_carve(out):
    """Plane groups are pairwise disjoint inside the workspace; offsets keep
    the kernels' alignment; frame f of a batch is at base + f * stride."""
    for p in every_plan(out):
        vol, hck, vck, hmn, vmn = sizes(out, p.W, p.H, p.D)
        assert (p.c_stride, p.vol_stride, p.hck_stride, p.vck_stride) == (vol, 4 * vol, hck, vck)
        assert p.b_volumes == 0
        nvol = {EIGHT: 8, FOUR: 4, PAIR: 2}[p.route]
        for f in range(p.frames):
            assert f * p.vol_stride + nvol * vol <= p.paths_bytes
        assert nvol * vol <= p.vol_stride or p.frames == 1
        if p.route == EIGHT:
            assert (p.b_ck, p.b_ckv, p.b_mn, p.ckpt_bytes) == (-1, -1, -1, 0)
            continue
        assert (p.b_ck, p.b_ckv) == (p.hck_off, p.vck_off)
        assert p.b_mn == (p.mn_off if p.minima else -1)
        spans = [(p.hck_off + f * p.hck_stride, hck) for f in range(p.frames)]
        spans += [(p.vck_off + f * p.vck_stride, vck) for f in range(p.frames)]
        if p.route == PAIR:
            # the kernels address the pair planes as planes 2 and 3 after CKV's two
            assert p.pair_off == p.vck_off + vck
            spans.append((p.pair_off, vck))
        if p.minima:
            spans.append((p.mn_off, hmn + vmn))
            assert p.mn_off % 8 == 0
        spans.sort()
        for (a, n), (b, _) in zip(spans, spans[1:]):
            assert a + n <= b, vars(p)
        assert spans[0][0] >= 0 and spans[-1][0] + spans[-1][1] <= p.ckpt_bytes, vars(p)
        for a, _ in spans[:len(spans) - (1 if p.minima else 0)]:
            assert a % p.D == 0, vars(p)


def test_reserve_covers_every_frame_plan(out):
    for p in out.plans["frame"]:
        paths, ckpt = out.reserve[(p.W, p.H, p.D)]
        assert p.paths_bytes <= paths and p.ckpt_bytes <= ckpt, vars(p)


def test_reserve_is_the_parents_expression(out):
    """sva_reserve sized paths = 4 * vol and ckpt = hck + vck (+ vck where the
    class has the pair route) (+ hmn + vmn where it has minima)."""
    shapes = [(W, H, D) for (W, H), D in itertools.product(SHAPES, NATIVE)]
    for W, H, D in shapes + [(65, 31, 100), (65, 31, 320)]:
        vol, hck, vck, hmn, vmn = sizes(out, W, H, D)
        ckpt = hck + vck + (vck if out.pair.get(D) else 0) + (hmn + vmn if out.minima.get(D) else 0)
        assert out.reserve[(W, H, D)] == (4 * vol, ckpt), (W, H, D)


def test_refusals(out):
    named = {k: v[0] for k, v in out.plans.items() if k.startswith(("ok_", "bad_"))}
    assert len(named) == 17
    for name, p in named.items():
        if name == "ok_pair":
            assert p.valid == out.pair[128]
        elif name == "ok_minima":
            assert p.valid == (out.minima[128] and out.seg[128] == 8)
        else:
            assert p.valid == name.startswith("ok_"), name
    assert named["bad_4g"].vol == 1 << 32 and named["ok_below_4g"].vol < 1 << 32
    assert named["bad_4g_frame"].vol == 1 << 32 and named["bad_4g_eight"].vol == 1 << 32
    # tile buffers present exactly on the tile routes, minima planes exactly with minima
    assert out.fit == [1, 0, 0, 0, 1, 1]
