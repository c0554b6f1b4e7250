"""Rectification and masking (§2.5g) without a GPU.

1. csrc/rectify_math.h through host programs with their own main, built under
   AddressSanitizer and UBSan and run directly: the per-pixel routine over whole
   small views, qx, qy, value and valid equal to tests/rectify_expect.py exactly;
   view_error's order; sva_rectify_view_of against the numpy form, bit for bit.
2. map_filter_args.h: the refusals of sva_rectify and sva_mask_maps, in order.
3. array_args.h: plan_views with the mask on for 1..4 devices, and the rules
   sva_array_depth_rectified adds to check_array_args.
4. include/sva.h: the new declarations, checked by a compile.
Nothing is loaded into Python under a sanitizer."""
import os
import struct
import subprocess

import numpy as np
import pytest

import rectify_expect as re_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereovisionarray_amd", "csrc")
INC = os.path.join(ROOT, "include")


def build(d, name, text):
    src = d / (name + ".cpp")
    src.write_text(text)
    exe = d / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-g", "-I", CSRC, "-I", INC, str(src), "-o",
                    str(exe)], check=True)
    return str(exe)


# ---- the expectation's own hand-checkable cases ------------------------------------
def test_identity_is_the_source():
    src = re_.texture(23, 17, 1)
    out, valid, qmap = re_.rectify_one(src, re_.view(), 23, 17, 9)
    assert np.array_equal(out, src) and valid.all()
    assert np.array_equal(qmap[..., 0], 32 * np.mgrid[0:17, 0:23][1])


def test_integer_translation_shifts_over_border():
    src = re_.texture(23, 17, 2)
    out, valid, _ = re_.rectify_one(src, re_.view([1, 0, 5, 0, 1, -3, 0, 0, 1]), 23, 17, 77)
    want = np.full_like(src, 77)
    want[3:, :18] = src[:14, 5:]
    ok = np.zeros_like(src)
    ok[3:, :18] = 1
    assert np.array_equal(out, want) and np.array_equal(valid, ok)


def test_half_pixel_is_the_rounded_mean():
    src = re_.texture(23, 17, 3)
    out, valid, _ = re_.rectify_one(src, re_.view([1, 0, 0.5, 0, 1, 0, 0, 0, 1]), 23, 17, 0)
    p = src.astype(int)
    assert np.array_equal(out[:, :-1], (p[:, :-1] + p[:, 1:] + 1) >> 1)
    assert valid[:, :-1].all() and not valid[:, -1].any()


def test_full_model_uses_every_fraction():
    v = re_.rolled(128, 96)
    _, valid, qmap = re_.rectify_one(re_.texture(128, 96, 4), v, 128, 96)
    assert valid.mean() > 0.9
    ok = valid != 0
    assert len(np.unique(qmap[..., 0][ok] & 31)) == 32 and len(np.unique(qmap[..., 1][ok] & 31)) == 32


# ---- the header's per-pixel routine -------------------------------------------------
PIXEL_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rectify_math.h"
using namespace sva;
// in:  i32 n_cases; per case i32 sw, sh, W, H, border; 18 f64 (the view); sw*sh u8
// out: per case and pixel i32 qx, qy, value, valid
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t n = 0;
    if (std::fread(&n, 4, 1, in) != 1) return 2;
    for (int c = 0; c < n; c++) {
        int32_t hd[5];
        sva_rectify_view v;
        static_assert(sizeof(v) == 18 * sizeof(double), "packed");
        if (std::fread(hd, 4, 5, in) != 5 || std::fread(&v, sizeof(v), 1, in) != 1) return 2;
        const int sw = hd[0], sh = hd[1], W = hd[2], H = hd[3];
        std::vector<uint8_t> src((size_t)sw * sh);
        if (std::fread(src.data(), 1, src.size(), in) != src.size()) return 2;
        const bool distort = rc::has_distortion(v);
        std::vector<int32_t> res;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                // at() faults under the sanitizer's eyes if the routine reads a tap it
                // judged outside
                const rc::Sample s = rc::sample(v, distort, x, y, sw, sh, (unsigned)hd[4],
                    [&](int X, int Y) { return src.at((size_t)Y * sw + (size_t)X); });
                res.insert(res.end(), {s.qx, s.qy, (int32_t)s.value, (int32_t)s.valid});
            }
        std::fwrite(res.data(), 4, res.size(), out);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
"""


def pixel_cases():
    """name -> (src, view, W, H, border)."""
    t = re_.texture(23, 17, 5)
    big = re_.texture(61, 45, 6)
    cases = {
        "identity": (t, re_.view(), 23, 17, 9),
        "translation": (t, re_.view([1, 0, 5, 0, 1, -3, 0, 0, 1]), 23, 17, 77),
        "half_pixel": (t, re_.view([1, 0, 0.5, 0, 1, 0, 0, 0, 1]), 23, 17, 0),
        "full_model": (big, re_.rolled(61, 45, roll_deg=0.7, k1=-0.12, k2=0.03, p1=1e-3, p2=-2e-3,
                                       k3=0.01, f=55.0), 53, 37, 200),
        "affine": (big, re_.rolled(61, 45, persp=(0, 0), k1=0.0), 53, 37, 3),
        "all_outside": (t, re_.view([1, 0, 500, 0, 1, 0, 0, 0, 1]), 23, 17, 41),
        # w = 1 - x / 8: positive, zero at x = 8, negative beyond
        "w_changes_sign": (t, re_.view([1, 0, 0, 0, 1, 0, -0.125, 0, 1]), 23, 17, 5),
        # sx = +-2^20 exactly at x = 1, just inside at x = 0
        "limit_plus": (t, re_.view([0.03125, 0, 1048575.96875, 0, 1, 0, 0, 0, 1]), 4, 3, 8),
        "limit_minus": (t, re_.view([-0.03125, 0, -1048575.96875, 0, 1, 0, 0, 0, 1]), 4, 3, 8),
        # 0 / 0 at (0, 0): h2 = h5 = h8 = 0 and w = x + y
        "nan": (t, re_.view([1, 0, 0, 0, 1, 0, 1, 1, 0]), 6, 5, 66),
        "huge": (t, re_.view([1e300, 0, 0, 0, 1e300, 0, 0, 0, 1]), 5, 4, 1),
        "distorted_to_infinity": (t, re_.view([1, 0, 0, 0, 1, 0, 0, 0, 1], 0, 0, 1e-3, 1e-3,
                                              (1e300, 0, 0, 0, 0)), 5, 4, 2),
    }
    return cases


def test_per_pixel_routine_equals_numpy(tmp_path):
    exe = build(tmp_path, "rectpix", PIXEL_PROGRAM)
    cases = pixel_cases()
    blob = struct.pack("<i", len(cases))
    for src, v, W, H, border in cases.values():
        sh, sw = src.shape
        blob += struct.pack("<5i", sw, sh, W, H, border) + re_.flat(v).tobytes() + src.tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    run = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                         capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    got = np.fromfile(tmp_path / "out.bin", np.int32)
    at = 0
    seen = {}
    for name, (src, v, W, H, border) in cases.items():
        g = got[at:at + 4 * W * H].reshape(H, W, 4)
        at += 4 * W * H
        out, valid, qmap = re_.rectify_one(src, v, W, H, border)
        assert np.array_equal(g[..., 0], qmap[..., 0]), name
        assert np.array_equal(g[..., 1], qmap[..., 1]), name
        assert np.array_equal(g[..., 2], out), name
        assert np.array_equal(g[..., 3], valid), name
        seen[name] = (out, valid, qmap)
    assert at == got.size
    # the cases are what they claim to be
    assert np.array_equal(seen["identity"][0], cases["identity"][0]) and seen["identity"][1].all()
    assert 0.5 < seen["full_model"][1].mean() < 1.0
    assert not seen["all_outside"][1].any() and (seen["all_outside"][0] == 41).all()
    assert (seen["all_outside"][2] != re_.OUTSIDE).all()       # inside the limits, off the source
    q = seen["w_changes_sign"][2][..., 0]
    assert (q[:, :8] != re_.OUTSIDE).all() and (q[:, 8:] == re_.OUTSIDE).all()
    for name in ("limit_plus", "limit_minus"):
        q = seen[name][2][..., 0]
        assert (q[:, 0] != re_.OUTSIDE).all() and (q[:, 1:] == re_.OUTSIDE).all(), name
    q = seen["nan"][2][..., 0]
    assert q[0, 0] == re_.OUTSIDE and (q.ravel()[1:] != re_.OUTSIDE).all()
    assert (seen["huge"][2][..., 0].ravel()[1:] == re_.OUTSIDE).all()


# ---- view_error, sva_rectify_view_of ---------------------------------------------------
VIEW_PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include "rectify_math.h"
using namespace sva;
int main(int argc, char** argv) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double inf = std::numeric_limits<double>::infinity();
    sva_rectify_view ok{{1, 0, 0, 0, 1, 0, 0, 0, 1}, 3, 4, 50, 60, 0, 0, 0, 0, 0};
    auto show = [](const sva_rectify_view& v) {
        const char* m = rc::view_error(v);
        std::printf("%s\n", m ? m : "ok");
    };
    show(ok);
    sva_rectify_view v = ok;
    v.k3 = nan; show(v);
    v.fy = 0; show(v);
    v.cx = inf; show(v);
    v.h[8] = nan; show(v);
    v = ok; v.fx = -1; show(v);
    v = ok; v.fx = inf; show(v);
    v = ok; v.cy = nan; v.p1 = inf; show(v);
    v = ok; v.h[0] = -inf; show(v);
    v = ok; v.k1 = 1e300; v.h[8] = 0; show(v);   // odd but finite: allowed
    // view_of: 9 + 5 + 9 + 9 doubles in, the status and the 18 doubles out
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (argc != 3 || !in || !out) return 2;
    double a[32];
    while (std::fread(a, 8, 32, in) == 32) {
        sva_rectify_view r;
        std::memset(&r, 0x5A, sizeof(r));
        const char* m = rc::view_of(a, a + 9, a + 14, a + 23, &r);
        const double status = m ? 1.0 : 0.0;
        std::fwrite(&status, 8, 1, out);
        std::fwrite(&r, sizeof(r), 1, out);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
"""


def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def test_view_error_order_and_view_of(tmp_path):
    exe = build(tmp_path, "rectview", VIEW_PROGRAM)
    rng = np.random.default_rng(3)
    rows = []
    for i in range(40):
        f, fi = rng.uniform(400, 2000, 2)
        K_raw = [f, 0, rng.uniform(300, 700), 0, f * rng.uniform(0.98, 1.02), rng.uniform(200, 500),
                 0, 0, 1]
        K_ideal = [fi, rng.uniform(-0.5, 0.5) if i % 3 == 0 else 0, rng.uniform(300, 700), 0, fi,
                   rng.uniform(200, 500), 0, 0, 1]
        R = rotation(*rng.uniform(-0.02, 0.02, 3)).ravel()
        dist = rng.uniform(-0.2, 0.2, 5) * (i % 4 != 0)
        rows.append(np.concatenate([K_raw, dist, R, K_ideal]))
    good = len(rows)
    eye = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    K = [800, 0, 320, 0, 800, 240, 0, 0, 1]

    def bad(K_raw=K, dist=(0,) * 5, R=eye, K_ideal=K):
        rows.append(np.concatenate([K_raw, dist, R, K_ideal]).astype(np.float64))
    bad(K_raw=[800, 0.1, 320, 0, 800, 240, 0, 0, 1])          # skew
    bad(K_raw=[800, 0, 320, 0.1, 800, 240, 0, 0, 1])
    bad(K_raw=[800, 0, 320, 0, 800, 240, 0, 0, 2])            # bottom row
    bad(K_raw=[800, 0, 320, 0, 800, 240, 1e-9, 0, 1])
    bad(K_ideal=[800, 0, 320, 0, 0, 240, 0, 0, 1])            # singular
    bad(K_ideal=[1, 2, 3, 2, 4, 6, 0, 0, 1])
    bad(dist=(0, np.nan, 0, 0, 0))
    bad(R=[1, 0, 0, 0, np.inf, 0, 0, 0, 1])
    bad(K_ideal=[800, 0, np.nan, 0, 800, 240, 0, 0, 1])
    np.stack(rows).astype(np.float64).tofile(tmp_path / "in.bin")
    run = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                         capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    h, c, f, k = ("rectify view: h has a non-finite entry", "rectify view: cx, cy must be finite",
                  "rectify view: fx, fy must be finite and > 0",
                  "rectify view: a distortion coefficient is not finite")
    assert run.stdout.splitlines() == ["ok", k, f, c, h, f, f, c, h, "ok"]
    got = np.fromfile(tmp_path / "out.bin", np.float64).reshape(len(rows), 19)
    for i, row in enumerate(rows):
        want = re_.view_of(row[:9], row[9:14], row[14:23], row[23:])
        if i >= good:
            assert want is None and got[i, 0] == 1.0, i
            # *out untouched where refused
            assert (got[i, 1:].view(np.uint64) == 0x5A5A5A5A5A5A5A5A).all(), i
            continue
        assert got[i, 0] == 0.0, i
        # bit for bit, in the documented order: no ulp allowance is needed
        assert np.array_equal(got[i, 1:].view(np.uint64), re_.flat(want).view(np.uint64)), i
    # and the product means what it says: h maps an ideal pixel to the raw pixel of its ray
    row = rows[1]
    v = re_.view_of(row[:9], row[9:14], row[14:23], row[23:])
    ray = row[14:23].reshape(3, 3) @ np.linalg.solve(row[23:].reshape(3, 3), [100.0, 50.0, 1.0])
    p = row[:9].reshape(3, 3) @ ray
    q = v["h"].reshape(3, 3) @ [100.0, 50.0, 1.0]
    assert np.allclose(p[:2] / p[2], q[:2] / q[2], rtol=0, atol=1e-8)


# ---- the refusals of the two argument groups ----------------------------------------------
ARGS_PROGRAM = r"""
#include <cstdio>
#include <limits>
#include <string>
#include <vector>
#include "map_filter_args.h"
using namespace sva;
static void show(const char* name, int st, const std::string& msg) {
    std::printf("%s|%d|%s\n", name, st, st ? msg.c_str() : "");
}
int main() {
    std::string msg;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<uint8_t> mem(1 << 16);
    uint8_t* p = mem.data();
    sva_rectify_view views[3];
    for (auto& v : views) v = sva_rectify_view{{1, 0, 0, 0, 1, 0, 0, 0, 1}, 0, 0, 1, 1, 0, 0, 0, 0, 0};
    // 3 views 20 x 10 (pitch 24) -> 16 x 8 (pitch 18): src 720 bytes, out 432, map 3072
    const RectifyArgs ok = {p, 3, 20, 10, 24, views, 16, 8, 18, 0, p + 1024, p + 2048,
                            (int32_t*)(p + 4096)};
    auto rect = [&](const char* name, RectifyArgs a) { show(name, check_rectify(a, msg), msg); };
    rect("ok", ok);
    { RectifyArgs a = ok; a.valid = nullptr; a.map = nullptr; rect("ok_bare", a); }
    { RectifyArgs a = ok; a.src = nullptr; a.n = 0; rect("null_src", a); }
    { RectifyArgs a = ok; a.views = nullptr; rect("null_views", a); }
    { RectifyArgs a = ok; a.out = nullptr; a.border = 256; rect("null_out", a); }
    { RectifyArgs a = ok; a.n = 0; a.src_w = 40000; rect("n_0", a); }
    { RectifyArgs a = ok; a.out_h = 0; a.src_w = 40000; rect("size_0", a); }
    { RectifyArgs a = ok; a.src_w = 32768; a.src_pitch = 1; rect("src_w_32768", a); }
    { RectifyArgs a = ok; a.out_h = 32768; rect("out_h_32768", a); }
    { RectifyArgs a = ok; a.src = p + 32768; a.src_w = 32767; a.src_pitch = 32767; a.n = 1; a.src_h = 1; rect("src_w_32767", a); }
    { RectifyArgs a = ok; a.src_pitch = 19; a.border = -1; rect("src_pitch", a); }
    { RectifyArgs a = ok; a.out_pitch = 15; rect("out_pitch", a); }
    { RectifyArgs a = ok; a.border = 256; a.out = p; rect("border_256", a); }
    { RectifyArgs a = ok; a.border = -1; rect("border_negative", a); }
    { RectifyArgs a = ok; a.out = p; views[1].fx = 0; rect("in_place", a); views[1].fx = 1; }
    { RectifyArgs a = ok; a.out = p + 715; rect("out_on_src_tail", a); }
    { RectifyArgs a = ok; a.out = p + 716; rect("out_after_src", a); }     // 29 * 24 + 20 = 716
    { RectifyArgs a = ok; a.valid = p + 1024 + 429; rect("valid_on_out_tail", a); }  // 23 * 18 + 16 = 430
    { RectifyArgs a = ok; a.valid = p + 1024 + 430; rect("valid_after_out", a); }
    { RectifyArgs a = ok; a.map = (int32_t*)(p + 700); rect("map_on_src", a); }
    { RectifyArgs a = ok; a.map = (int32_t*)(p + 1452); rect("map_on_out", a); }
    { RectifyArgs a = ok; views[2].k1 = nan; views[1].h[3] = nan; rect("view_1_h", a); views[1].h[3] = 0; }
    rect("view_2_k", ok);
    views[2].k1 = 0;
    views[0].cx = nan;
    rect("view_0_c", ok);
    views[0].cx = 0;
    // sva_mask_maps: 2 maps 6 x 4: u16 planes 96 bytes, f32 192, valid 48
    uint16_t* d = (uint16_t*)p;
    float* s = (float*)(p + 256);
    const MaskArgs mok = {{d, s, 2, 6, 4, 0xFFFF, (uint16_t*)(p + 1024), (float*)(p + 2048)}, p + 512};
    auto mask = [&](const char* name, MaskArgs a) { show(name, check_mask(a, msg), msg); };
    mask("mask_ok", mok);
    { MaskArgs a = mok; a.m.out = d; a.m.out_sub = s; mask("mask_in_place", a); }
    { MaskArgs a = mok; a.m.subpix = nullptr; a.m.out_sub = nullptr; mask("mask_bare", a); }
    { MaskArgs a = mok; a.valid = nullptr; a.m.n = 0; mask("mask_null_valid", a); }
    { MaskArgs a = mok; a.m.disps = nullptr; mask("mask_null_disps", a); }
    { MaskArgs a = mok; a.m.out = nullptr; mask("mask_null_out", a); }
    { MaskArgs a = mok; a.m.n = 0; a.m.W = 0; mask("mask_n_0", a); }
    { MaskArgs a = mok; a.m.H = 0; a.m.subpix = nullptr; mask("mask_size_0", a); }
    { MaskArgs a = mok; a.m.W = 65536; a.m.H = 32768; a.m.subpix = nullptr; mask("mask_2_31", a); }
    { MaskArgs a = mok; a.m.subpix = nullptr; a.m.out = d + 1; mask("mask_out_sub_alone", a); }
    { MaskArgs a = mok; a.m.out = d + 1; mask("mask_out_shifted", a); }
    { MaskArgs a = mok; a.m.out = (uint16_t*)(p + 512 + 46); mask("mask_out_on_valid", a); }
    { MaskArgs a = mok; a.m.out = (uint16_t*)(p + 512 + 48); mask("mask_out_after_valid", a); }
    { MaskArgs a = mok; a.m.out_sub = (float*)(p + 1024 + 92); mask("mask_out_sub_on_out", a); }
    return 0;
}
"""


def test_refusals_of_the_argument_groups(tmp_path):
    exe = build(tmp_path, "rectargs", ARGS_PROGRAM)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    got = [tuple(line.split("|")) for line in run.stdout.splitlines()]
    INV, UNS = "1", "2"
    null, size, big, pitch, border = ("null pointer", "image size must be positive",
                                      "rectification takes widths and heights up to 32767",
                                      "pitch < width", "border must be 0..255")
    over = "an output overlaps the source or another output (in place is not offered)"
    inpl = ("an output overlaps an input or another output (in place: out == disps, "
            "out_sub == subpix)")
    want = [
        ("ok", "0", ""), ("ok_bare", "0", ""), ("null_src", INV, null), ("null_views", INV, null),
        ("null_out", INV, null), ("n_0", INV, "n must be >= 1"), ("size_0", INV, size),
        ("src_w_32768", UNS, big), ("out_h_32768", UNS, big), ("src_w_32767", "0", ""),
        ("src_pitch", INV, pitch), ("out_pitch", INV, pitch), ("border_256", INV, border),
        ("border_negative", INV, border), ("in_place", INV, over), ("out_on_src_tail", INV, over),
        ("out_after_src", "0", ""), ("valid_on_out_tail", INV, over), ("valid_after_out", "0", ""),
        ("map_on_src", INV, over), ("map_on_out", INV, over),
        ("view_1_h", INV, "rectify view: h has a non-finite entry (view 1)"),
        ("view_2_k", INV, "rectify view: a distortion coefficient is not finite (view 2)"),
        ("view_0_c", INV, "rectify view: cx, cy must be finite (view 0)"),
        ("mask_ok", "0", ""), ("mask_in_place", "0", ""), ("mask_bare", "0", ""),
        ("mask_null_valid", INV, null), ("mask_null_disps", INV, null),
        ("mask_null_out", INV, null), ("mask_n_0", INV, "n_maps must be >= 1"),
        ("mask_size_0", INV, size), ("mask_2_31", UNS, "masking needs W * H < 2^31"),
        ("mask_out_sub_alone", INV, "out_sub needs subpix"), ("mask_out_shifted", INV, inpl),
        ("mask_out_on_valid", INV, inpl), ("mask_out_after_valid", "0", ""),
        ("mask_out_sub_on_out", INV, inpl),
    ]
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w]


# ---- the frame: view planning with the mask on, the entry's rules --------------------------
FRAME_PROGRAM = r"""
#include <cstdio>
#include <limits>
#include <set>
#include <string>
#include <vector>
#include "array_args.h"
using namespace sva;
#define REQUIRE(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)
int main() {
    // nine groups, camera g against camera g + 1 (mod 9); the mask (refs_on_0)
    // needs every reference view, which is every view, on device 0
    std::vector<sva_array_pair> pairs;
    std::vector<int> group_of;
    for (int g = 0; g < 9; g++) {
        sva_array_pair p{};
        p.ref = g;
        p.other = (g + 1) % 9;
        pairs.push_back(p);
        group_of.push_back(g);
    }
    const int n_pairs = (int)pairs.size();
    for (int nd = 1; nd <= 4; nd++) {
        std::vector<int32_t> dev_of(n_pairs);
        for (int j = 0; j < n_pairs; j++) dev_of[j] = group_of[j] % nd;
        std::vector<std::vector<int>> slot, base;
        std::vector<int> n_need, base_need;
        std::vector<char> used, base_used;
        plan_views(nd, 9, pairs.data(), n_pairs, dev_of.data(), true, slot, n_need, used);
        plan_views(nd, 9, pairs.data(), n_pairs, dev_of.data(), false, base, base_need, base_used);
        REQUIRE(n_need[0] == 9);
        std::set<int> slots;
        for (int v = 0; v < 9; v++) {
            REQUIRE(used[v] && slot[0][v] >= 0 && slot[0][v] < 9 && slots.insert(slot[0][v]).second);
            REQUIRE(base[0][v] < 0 ? slot[0][v] >= base_need[0] : slot[0][v] == base[0][v]);
        }
        for (int d = 1; d < nd; d++) REQUIRE(slot[d] == base[d]);
        std::printf("%d %d\n", nd, base_need[0]);
    }
    // the entry's rules, after the smoothed entry's
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
    const double nan = std::numeric_limits<double>::quiet_NaN();
    // {wmed_radius, wmed_min_support, wmed_select, null rect, bad view (1 + index, 0: none),
    //  border, mask}
    const int rows[][7] = {{5, 1, 0, 0, 0, 0, 1},   {0, 1, 0, 0, 0, 255, 0}, {16, 1, 0, 1, 0, 0, 0},
                           {0, 0, 0, 1, 0, 0, 0},   {0, 1, 2, 1, 0, 0, 0},   {0, 1, 0, 1, 2, 256, 2},
                           {0, 1, 0, 0, 2, 256, 2}, {0, 1, 0, 0, 1, 0, 0},   {0, 1, 0, 0, 0, 256, 2},
                           {0, 1, 0, 0, 0, -1, 0},  {0, 1, 0, 0, 0, 0, 2},   {0, 1, 0, 0, 0, 0, -1}};
    for (const auto& r : rows) {
        sva_rectify_view rv[2];
        for (auto& v : rv) v = sva_rectify_view{{1, 0, 0, 0, 1, 0, 0, 0, 1}, 0, 0, 1, 1, 0, 0, 0, 0, 0};
        if (r[4]) rv[r[4] - 1].fy = nan;
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
        a.wmed = r[0] != 0;
        a.wmed_radius = r[0];
        a.wmed_min_support = r[1];
        a.wmed_select = r[2];
        a.rect = true;
        a.rect_views = r[3] ? nullptr : rv;
        a.rect_border = r[5];
        a.rect_mask = r[6];
        std::string msg;
        std::vector<int32_t> ratio;
        const int st = check_array_args(a, msg, ratio);
        std::printf("%d|%s\n", st, st ? msg.c_str() : "");
    }
    return 0;
}
"""


def test_view_planning_with_the_mask_and_the_entry_rules(tmp_path):
    exe = build(tmp_path, "rectframe", FRAME_PROGRAM)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    lines = run.stdout.splitlines()
    # what device 0 holds without the mask, worked by hand for this rig: everything
    # with one device; with two, groups 0 2 4 6 8 name every view; with three, groups
    # 0 3 6 name views 0 1 3 4 6 7; with four, groups 0 4 8 name 0 1 4 5 8.  With the
    # mask it holds all nine (the program checks), the old slots unchanged
    assert lines[:4] == ["1 9", "2 9", "3 6", "4 5"]
    got = [tuple(line.split("|")) for line in lines[4:]]
    f = "rectify view: fx, fy must be finite and > 0"
    want = [("0", ""), ("0", ""), ("1", "wmed radius must be 1..15"),
            ("1", "wmed min_support must be 1..961"), ("1", "wmed select must be 0 or 1"),
            ("1", "null rect"), ("1", f + " (view 1)"), ("1", f + " (view 0)"),
            ("1", "border must be 0..255"), ("1", "border must be 0..255"),
            ("1", "mask must be 0 or 1"), ("1", "mask must be 0 or 1")]
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w]


# ---- the declarations -------------------------------------------------------------------
DECL_PROGRAM = r"""
#include "sva.h"
int main(void) {
    int (*a)(void*, const uint8_t*, int, int, int, size_t, const sva_rectify_view*, int, int, size_t,
             int, uint8_t*, uint8_t*, int32_t*) = sva_rectify_d;
    int (*b)(void*, const uint8_t*, int, int, int, size_t, const sva_rectify_view*, int, int, size_t,
             int, uint8_t*, uint8_t*, int32_t*) = sva_rectify;
    int (*c)(void*, const uint16_t*, const float*, int, int, int, const uint8_t*, uint16_t,
             uint16_t*, float*) = sva_mask_maps_d;
    int (*d)(void*, const uint16_t*, const float*, int, int, int, const uint8_t*, uint16_t,
             uint16_t*, float*) = sva_mask_maps;
    int (*e)(const double*, const double*, const double*, const double*, sva_rectify_view*) =
        sva_rectify_view_of;
    int (*f)(void*, const uint8_t* const*, int, int, int, size_t, const sva_array_pair*, int,
             const int32_t*, int, int, const double*, double, double, int, int, double*, uint8_t*,
             uint8_t*, float*, uint16_t*, uint16_t*, uint16_t*, const int32_t*, int, int, int, int,
             uint8_t*, uint8_t*, int, int, int, uint32_t*, int, int, int, uint8_t*, int,
             const uint16_t*, int, int, uint16_t*, const sva_rectify_view*, int, int, uint8_t*,
             uint8_t*) = sva_array_depth_rectified;
    (void)a; (void)b; (void)c; (void)d; (void)e; (void)f;
    return sizeof(sva_rectify_view) == 144 && SVA_ABI_VERSION == 6 && SVA_RECTIFY_MAX_SIZE == 32767
               ? 0 : 1;
}
"""


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", ".c"), ("g++", "-std=c++17", ".cpp")])
def test_declarations_compile(tmp_path, compiler, std, ext):
    src = tmp_path / ("decl" + ext)
    src.write_text(DECL_PROGRAM)
    subprocess.run([compiler, std, "-Wall", "-Werror", "-c", "-I", INC, str(src), "-o",
                    str(tmp_path / "decl.o")], check=True)
