// The C++ mirror of rectification (include/sva.hpp: rectifyViewOf, rectifyViews,
// maskMaps, computeArrayDepthRectified) on a GPU.  Built
// and run by tests/test_rectify_cpp_gpu.py.  rectifyViews must equal the C entry
// it wraps, plane for plane, and a pixel walk of the rule written here; the frame
// must equal the C entry and the composition of the wrappers.
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#include "sva.hpp"

static int failures = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c);    \
            failures++;                                                 \
        }                                                               \
    } while (0)

using namespace sva;

template <typename T>
static bool same_bits(const std::vector<T>& a, const T* b) {
    return std::memcmp(a.data(), b, a.size() * sizeof(T)) == 0;
}

// One view by the rule, pixel by pixel (built with -ffp-contract=off: every
// operation is rounded on its own).
static void walk(const std::vector<uint8_t>& src, int sw, int sh, const sva_rectify_view& v, int W,
                 int H, int border, std::vector<uint8_t>& out, std::vector<uint8_t>& valid,
                 std::vector<int32_t>& map) {
    out.assign((size_t)W * H, 0);
    valid.assign((size_t)W * H, 0);
    map.assign((size_t)W * H * 2, 0);
    const bool plain = v.k1 == 0 && v.k2 == 0 && v.p1 == 0 && v.p2 == 0 && v.k3 == 0;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
#define R(e) (e)
            const double w = R(R(R(v.h[6] * x) + R(v.h[7] * y)) + v.h[8]);
            double sx = R(R(R(R(v.h[0] * x) + R(v.h[1] * y)) + v.h[2]) / w);
            double sy = R(R(R(R(v.h[3] * x) + R(v.h[4] * y)) + v.h[5]) / w);
            if (!plain) {
                const double xn = R(R(sx - v.cx) / v.fx), yn = R(R(sy - v.cy) / v.fy);
                const double xx = R(xn * xn), yy = R(yn * yn), xy = R(xn * yn), r2 = R(xx + yy);
                const double rad =
                    R(1.0 + R(r2 * R(v.k1 + R(r2 * R(v.k2 + R(r2 * v.k3))))));
                const double xd = R(R(R(xn * rad) + R(R(2.0 * v.p1) * xy)) +
                                    R(v.p2 * R(r2 + R(2.0 * xx))));
                const double yd = R(R(R(yn * rad) + R(v.p1 * R(r2 + R(2.0 * yy)))) +
                                    R(R(2.0 * v.p2) * xy));
                sx = R(R(xd * v.fx) + v.cx);
                sy = R(R(yd * v.fy) + v.cy);
            }
#undef R
            const size_t p = (size_t)y * W + x;
            const double L = 1048576.0;
            if (!(w > 0 && sx > -L && sx < L && sy > -L && sy < L)) {
                out[p] = (uint8_t)border;
                map[2 * p] = map[2 * p + 1] = std::numeric_limits<int32_t>::min();
                continue;
            }
            const int qx = (int)std::nearbyint(sx * 32.0), qy = (int)std::nearbyint(sy * 32.0);
            const int X = (int)std::floor(qx / 32.0), Y = (int)std::floor(qy / 32.0);
            const int a = qx - 32 * X, b = qy - 32 * Y;
            int sum = 512;
            bool ok = true;
            for (int j = 0; j < 2; j++)
                for (int i = 0; i < 2; i++) {
                    const int wt = (i ? a : 32 - a) * (j ? b : 32 - b);
                    if (!wt) continue;
                    const bool in = X + i >= 0 && X + i < sw && Y + j >= 0 && Y + j < sh;
                    sum += wt * (in ? src[(size_t)(Y + j) * sw + X + i] : border);
                    ok = ok && in;
                }
            out[p] = (uint8_t)(sum >> 10);
            valid[p] = ok ? 1 : 0;
            map[2 * p] = qx;
            map[2 * p + 1] = qy;
        }
}

static sva_rectify_view model(int W, int H, double roll_deg, double tx, double ty, double k1,
                              double p1 = 0) {
    const double cx = (W - 1) / 2.0, cy = (H - 1) / 2.0, t = roll_deg * 3.14159265358979323846 / 180;
    const double c = std::cos(t), s = std::sin(t);
    sva_rectify_view v{};
    const double h[9] = {c, -s, cx - c * cx + s * cy + tx, s, c, cy - s * cx - c * cy + ty, 1e-5,
                         -2e-5, 1.0};
    std::copy(h, h + 9, v.h);
    v.cx = cx;
    v.cy = cy;
    v.fx = v.fy = W;
    v.k1 = k1;
    v.p1 = p1;
    return v;
}

static sva_rectify_view identity_view() {
    sva_rectify_view v{};
    v.h[0] = v.h[4] = v.h[8] = 1;
    v.fx = v.fy = 1;
    return v;
}

int main() {
    // ---- rectifyViewOf: the documented order, restated
    {
        const std::array<double, 9> Kr = {810.5, 0, 322.25, 0, 807.75, 241.5, 0, 0, 1};
        const std::array<double, 9> Ki = {800, 0.25, 320, 0, 800, 240, 0, 0, 1};
        const double cz = std::cos(0.01), sz = std::sin(0.01);
        const std::array<double, 9> R = {cz, -sz, 0.002, sz, cz, -0.001, -0.002, 0.001, 1};
        const std::array<double, 5> dist = {-0.11, 0.02, 1e-3, -2e-3, 0.005};
        const sva_rectify_view v = rectifyViewOf(Kr, dist, R, Ki);
        const double* k = Ki.data();
        volatile double c[9] = {k[4] * k[8] - k[5] * k[7], k[2] * k[7] - k[1] * k[8],
                                k[1] * k[5] - k[2] * k[4], k[5] * k[6] - k[3] * k[8],
                                k[0] * k[8] - k[2] * k[6], k[2] * k[3] - k[0] * k[5],
                                k[3] * k[7] - k[4] * k[6], k[1] * k[6] - k[0] * k[7],
                                k[0] * k[4] - k[1] * k[3]};
        volatile double det = k[0] * c[0];
        det = det + k[1] * c[3];
        det = det + k[2] * c[6];
        double inv[9], m[9], h[9];
        for (int i = 0; i < 9; i++) inv[i] = c[i] / det;
        auto mul = [](const double* a, const double* b, double* o) {
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) {
                    volatile double s = a[3 * i] * b[j];
                    volatile double u = a[3 * i + 1] * b[3 + j];
                    s = s + u;
                    u = a[3 * i + 2] * b[6 + j];
                    o[3 * i + j] = s + u;
                }
        };
        mul(R.data(), inv, m);
        mul(Kr.data(), m, h);
        CHECK(std::memcmp(h, v.h, sizeof(h)) == 0);
        CHECK(v.cx == 322.25 && v.cy == 241.5 && v.fx == 810.5 && v.fy == 807.75);
        CHECK(v.k1 == -0.11 && v.k2 == 0.02 && v.p1 == 1e-3 && v.p2 == -2e-3 && v.k3 == 0.005);
        bool threw = false;
        try {
            rectifyViewOf({810.5, 0.5, 322.25, 0, 807.75, 241.5, 0, 0, 1}, dist, R, Ki);
        } catch (const Error&) {
            threw = true;
        }
        CHECK(threw);
        threw = false;
        try {
            rectifyViewOf(Kr, dist, R, {1, 2, 3, 2, 4, 6, 0, 0, 1});
        } catch (const Error&) {
            threw = true;
        }
        CHECK(threw);
    }
    // ---- rectifyViews: three models, 53 x 37 from 61 x 45 views of pitch 64
    std::mt19937 rng(7);
    Engine eng(0);
    {
        const int sw = 61, sh = 45, W = 53, H = 37, n = 3, pitch = 64, border = 200;
        std::vector<std::vector<uint8_t>> img(n, std::vector<uint8_t>((size_t)pitch * sh, 0xEE));
        std::vector<std::vector<uint8_t>> packed(n, std::vector<uint8_t>((size_t)sw * sh));
        std::vector<ImageView> raw;
        for (int k = 0; k < n; k++) {
            for (int y = 0; y < sh; y++)
                for (int x = 0; x < sw; x++)
                    img[k][(size_t)y * pitch + x] = packed[k][(size_t)y * sw + x] =
                        (uint8_t)(96 + 60 * std::sin(x / 5.0 + k) * std::cos(y / 7.0) + rng() % 40);
            raw.emplace_back(img[k].data(), sw, sh, (size_t)pitch);
        }
        std::vector<sva_rectify_view> rect = {model(sw, sh, 0.7, 2, -1.5, -0.12, 1e-3),
                                              model(sw, sh, -1.1, -3.25, 2.5, 0), identity_view()};
        rect[2].h[2] = 0.5;
        const Rectified got = rectifyViews(eng, raw, rect, W, H, border, true);
        CHECK(got.views.size() == 3 && got.valid.size() == 3 && got.map.size() == 3);
        std::vector<uint8_t> src, c_out((size_t)W * H * n), c_valid((size_t)W * H * n);
        for (auto& p : packed) src.insert(src.end(), p.begin(), p.end());
        std::vector<int32_t> c_map((size_t)W * H * n * 2);
        eng.check(sva_rectify(eng.handle(), src.data(), n, sw, sh, sw, rect.data(), W, H, W, border,
                              c_out.data(), c_valid.data(), c_map.data()));
        long n_valid = 0;
        for (int k = 0; k < n; k++) {
            std::vector<uint8_t> out, valid;
            std::vector<int32_t> map;
            walk(packed[k], sw, sh, rect[k], W, H, border, out, valid, map);
            CHECK(got.views[k] == out);
            CHECK(got.valid[k] == valid);
            CHECK(got.map[k] == map);
            CHECK(same_bits(got.views[k], c_out.data() + (size_t)k * W * H));
            CHECK(same_bits(got.valid[k], c_valid.data() + (size_t)k * W * H));
            CHECK(same_bits(got.map[k], c_map.data() + (size_t)k * W * H * 2));
            for (uint8_t b : valid) n_valid += b;
        }
        CHECK(n_valid > W * H && n_valid < 3L * W * H);
        const Rectified bare = rectifyViews(eng, raw, rect);
        CHECK(bare.views.size() == 3 && bare.views[0].size() == (size_t)sw * sh && bare.map.empty());
        bool threw = false;
        try {
            rectifyViews(eng, raw, {rect[0]});
        } catch (const Error&) {
            threw = true;
        }
        CHECK(threw);
        rect[1].fx = 0;
        threw = false;
        try {
            rectifyViews(eng, raw, rect);
        } catch (const Error& e) {
            threw = std::string(e.what()).find("view 1") != std::string::npos;
        }
        CHECK(threw);
        // ---- maskMaps
        std::vector<std::vector<uint16_t>> maps(n, std::vector<uint16_t>((size_t)W * H));
        std::vector<std::vector<float>> sub(n, std::vector<float>((size_t)W * H));
        for (int k = 0; k < n; k++)
            for (size_t p = 0; p < maps[k].size(); p++) {
                maps[k][p] = (uint16_t)(rng() % 60);
                sub[k][p] = maps[k][p] + 0.25f;
            }
        const MaskedMaps mm = maskMaps(eng, maps, sub, got.valid, W, H);
        const MaskedMaps m8 = maskMaps(eng, maps, {}, got.valid, W, H, 255);
        CHECK(mm.maps.size() == 3 && mm.subpix.size() == 3 && m8.subpix.empty());
        for (int k = 0; k < n; k++)
            for (size_t p = 0; p < maps[k].size(); p++) {
                const bool ok = got.valid[k][p] != 0;
                if (mm.maps[k][p] != (ok ? maps[k][p] : 0xFFFF) ||
                    m8.maps[k][p] != (ok ? maps[k][p] : 255) ||
                    (ok ? mm.subpix[k][p] != sub[k][p] : !std::isnan(mm.subpix[k][p]))) {
                    CHECK(!"maskMaps follows valid");
                    break;
                }
            }
        threw = false;
        try {
            maskMaps(eng, maps, {}, {got.valid[0]}, W, H);
        } catch (const Error&) {
            threw = true;
        }
        CHECK(threw);
    }
    // ---- the frame.  The 5x5 rig of test_wmed.cpp: 5 px per grid unit
    {
        const int FW = 96, FH = 80, shift = 5;
        const double ps = 0.036 / FW;
        const size_t fnp = (size_t)FW * FH;
        std::vector<Camera> cams;
        for (int y = 0; y < 5; y++)
            for (int x = 0; x < 5; x++)
                cams.emplace_back(0.05, Point3d{-0.1 + x * 0.05, -0.1 + y * 0.05, -0.75}, ps);
        const int TW = FW + 4 * shift, TH = FH + 4 * shift;
        std::vector<uint8_t> tex((size_t)TW * TH);
        for (auto& px : tex) px = (uint8_t)(rng() & 255);
        std::vector<std::vector<uint8_t>> imgs(25, std::vector<uint8_t>(fnp));
        for (int c = 0; c < 25; c++) {
            const int gx = c % 5 - 2, gy = c / 5 - 2;
            for (int y = 0; y < FH; y++)
                for (int x = 0; x < FW; x++)
                    imgs[c][(size_t)y * FW + x] =
                        tex[(size_t)(y + (gy + 2) * shift) * TW + x + (gx + 2) * shift];
        }
        std::vector<ImageView> views;
        for (auto& im : imgs) views.emplace_back(im.data(), FW, FH);
        std::vector<sva_rectify_view> rect, same(25, identity_view());
        for (int c = 0; c < 25; c++)
            rect.push_back(model(FW, FH, 0.1 * (c % 7) - 0.3, 0.25 * (c % 5) - 0.5, 0.5 - 0.125 * (c % 9),
                                 0.01 * (c % 3)));
        MultiEngine me({0}, 2, SVA_MULTI_GATHER_PEER);
        sva_sgm_params q;
        sva_sgm_params_default(&q);
        q.D = 64;
        const int refs[3] = {12, 7, 11};
        std::vector<std::array<int, 2>> pairs;
        for (int r : refs)
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++)
                    if (dx || dy) pairs.push_back({r, r + dy * 5 + dx});
        const std::array<uint16_t, 256> w32 = wmedWeights(32);
        const int max_size = 30, max_diff = 1, max_dist = 12, min_found = 3, r = 3;
        auto frame = [&](const std::vector<sva_rectify_view>& rv, int radius, bool mask,
                         std::vector<std::vector<uint16_t>>* maps,
                         std::vector<std::vector<uint8_t>>* vw, std::vector<std::vector<uint8_t>>* vd) {
            return computeArrayDepthRectified(me, views, rv, cams, pairs, q, radius, &w32, 2, false,
                                              max_dist, min_found, SVA_FILL_MEDIAN, max_size, max_diff,
                                              SVA_ARRAY_GROUPS, true, false, 1, 2, 0, 0,
                                              SVA_FUSE_MEDIAN, 0.05, 9, mask, maps, vw, vd);
        };
        // identity and no mask: the smoothed wrapper; radius 0: the filled wrapper
        std::vector<std::vector<uint16_t>> m_id, m_sm, m_off, m_fl;
        std::vector<std::vector<uint8_t>> vw, vd;
        auto d_id = frame(same, r, false, &m_id, &vw, &vd);
        auto d_sm = computeArrayDepthSmoothed(me, views, cams, pairs, q, r, &w32, 2, false, max_dist,
                                              min_found, SVA_FILL_MEDIAN, max_size, max_diff,
                                              SVA_ARRAY_GROUPS, true, false, 1, 2, 0, 0,
                                              SVA_FUSE_MEDIAN, 0.05, &m_sm);
        CHECK(d_id == d_sm && m_id == m_sm && vw.size() == 25 && vd.size() == 25);
        for (int c : {12, 6, 18}) CHECK(vw[c] == imgs[c] && vd[c] == std::vector<uint8_t>(fnp, 1));
        CHECK(vw[0] == std::vector<uint8_t>(fnp, 0));   // camera 0 is in no pair
        auto d_off = frame(same, 0, false, &m_off, nullptr, nullptr);
        auto d_fl = computeArrayDepthFilled(me, views, cams, pairs, q, max_dist, min_found,
                                            SVA_FILL_MEDIAN, max_size, max_diff, SVA_ARRAY_GROUPS,
                                            true, false, 1, 2, 0, 0, SVA_FUSE_MEDIAN, 0.05, &m_fl);
        CHECK(d_off == d_fl && m_off == m_fl && m_off != m_id);
        // a real model, no mask: the smoothed wrapper on rectifyViews' views
        std::vector<std::vector<uint16_t>> m_rc, m_cmp, m_msk;
        auto d_rc = frame(rect, r, false, &m_rc, &vw, &vd);
        const Rectified alone = rectifyViews(eng, views, rect, 0, 0, 9);
        for (int c : {12, 6, 18, 7, 11}) CHECK(vw[c] == alone.views[c] && vd[c] == alone.valid[c]);
        std::vector<ImageView> rviews;
        for (auto& im : alone.views) rviews.emplace_back(im.data(), FW, FH);
        auto d_cmp = computeArrayDepthSmoothed(me, rviews, cams, pairs, q, r, &w32, 2, false, max_dist,
                                               min_found, SVA_FILL_MEDIAN, max_size, max_diff,
                                               SVA_ARRAY_GROUPS, true, false, 1, 2, 0, 0,
                                               SVA_FUSE_MEDIAN, 0.05, &m_cmp);
        CHECK(d_rc == d_cmp && m_rc == m_cmp && m_rc != m_id);
        // the mask changes the maps where the reference view is not valid
        auto d_msk = frame(rect, r, true, &m_msk, nullptr, nullptr);
        CHECK(d_msk.size() == 3 && m_msk.size() == 3 && m_msk != m_rc);
        bool threw = false;
        try {
            computeArrayDepthRectified(me, views, {rect[0]}, cams, pairs, q);
        } catch (const Error&) {
            threw = true;
        }
        CHECK(threw);
    }
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("rectify mirror ok\n");
    return 0;
}
