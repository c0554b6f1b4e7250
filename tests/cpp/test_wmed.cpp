// The C++ mirror of the weighted median filter (include/sva.hpp: wmedWeights,
// weightedMedian, computeArrayDepthSmoothed) on a GPU.  Built and run by
// tests/test_wmed_cpp_gpu.py.  weightedMedian must equal the C entry it wraps,
// plane for plane, and a pixel walk of the rule written here.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <tuple>

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

// One map by the rule, pixel by pixel: out, support and the source index (-1: not written).
static void walk(const std::vector<uint16_t>& d, const uint8_t* g, size_t pitch,
                 const uint16_t* w, const uint8_t* sel, int W, int H, int r, int min_support,
                 bool fill, std::vector<uint16_t>& out, std::vector<uint16_t>& support,
                 std::vector<long>& src) {
    auto ok = [&](size_t p) { return d[p] != 0xFFFF && d[p] != 0; };
    out = d;
    support.assign(d.size(), 0);
    src.assign(d.size(), -1);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * W + x;
            if ((sel && !sel[p]) || (!fill && !ok(p))) continue;
            std::vector<std::tuple<int, int, int, unsigned>> c;     // d, qy, qx, weight
            for (int qy = std::max(0, y - r); qy <= std::min(H - 1, y + r); qy++)
                for (int qx = std::max(0, x - r); qx <= std::min(W - 1, x + r); qx++) {
                    const size_t q = (size_t)qy * W + qx;
                    if (!ok(q)) continue;
                    const unsigned wq =
                        g ? w[std::abs((int)g[y * pitch + x] - (int)g[qy * pitch + qx])] : 1u;
                    if (wq) c.emplace_back((int)d[q], qy, qx, wq);
                }
            std::sort(c.begin(), c.end());
            support[p] = (uint16_t)c.size();
            if ((int)c.size() < min_support || c.empty()) continue;
            unsigned long long total = 0, run = 0;
            for (auto& e : c) total += std::get<3>(e);
            for (auto& e : c) {
                run += std::get<3>(e);
                if (2 * run >= total) {
                    out[p] = (uint16_t)std::get<0>(e);
                    src[p] = (long)std::get<1>(e) * W + std::get<2>(e);
                    break;
                }
            }
        }
}

int main() {
    const std::array<uint16_t, 256> w32 = wmedWeights(32), w8 = wmedWeights(8);
    CHECK(w32[0] == 1024 && w32[32] == 377 && w32[255] == 0 && w8[8] == 377 && w8[62] == 0);
    for (int i = 0; i < 256; i++)
        CHECK(w32[i] == (uint16_t)std::lround(1024.0 * std::exp(-i / 32.0)));
    bool threw = false;
    try {
        wmedWeights(0.0);
    } catch (const Error&) {
        threw = true;
    }
    CHECK(threw);

    const int W = 45, H = 19, n = 3, pitch = W + 3;
    const size_t np = (size_t)W * H;
    std::mt19937 rng(11);
    std::vector<std::vector<uint16_t>> maps(n, std::vector<uint16_t>(np));
    std::vector<std::vector<float>> sub(n, std::vector<float>(np));
    std::vector<std::vector<uint8_t>> sel(n, std::vector<uint8_t>(np)), gimg(n);
    std::vector<ImageView> guides;
    for (int k = 0; k < n; k++) {
        for (size_t p = 0; p < np; p++) {
            const unsigned v = rng() % 10;
            maps[k][p] = v < 2 ? (v ? 0xFFFF : 0) : (uint16_t)(1 + rng() % 9);
            sub[k][p] = (float)(k * np + p) + 0.5f;
            sel[k][p] = (uint8_t)(rng() % 3 ? 1 + rng() % 200 : 0);
        }
        gimg[k].assign((size_t)pitch * H, 0xEE);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) gimg[k][(size_t)y * pitch + x] = (uint8_t)((rng() % 4) * 20);
    }
    for (int k = 0; k < n; k++) guides.emplace_back(gimg[k].data(), W, H, (size_t)pitch);

    Engine eng(0);
    struct Case { int r, ms; bool fill, guided, selected, subpix; };
    const Case cases[] = {{2, 1, true, true, false, true},   {5, 3, false, true, true, true},
                          {1, 1, true, false, false, false}, {15, 40, true, false, true, true},
                          {7, 100, false, true, false, false}};
    for (const Case& c : cases) {
        const MedianFiltered got = weightedMedian(
            eng, maps, c.subpix ? sub : std::vector<std::vector<float>>{},
            c.guided ? guides : std::vector<ImageView>{}, c.guided ? &w8 : nullptr, W, H, c.r, c.ms,
            c.fill, c.selected ? sel : std::vector<std::vector<uint8_t>>{});
        CHECK(got.maps.size() == (size_t)n && got.support.size() == (size_t)n);
        CHECK(got.subpix.size() == (c.subpix ? (size_t)n : 0));
        long written = 0;
        for (int k = 0; k < n; k++) {
            std::vector<uint16_t> out, support;
            std::vector<long> src;
            walk(maps[k], c.guided ? gimg[k].data() : nullptr, pitch, w8.data(),
                 c.selected ? sel[k].data() : nullptr, W, H, c.r, c.ms, c.fill, out, support, src);
            CHECK(got.maps[k] == out);
            CHECK(got.support[k] == support);
            for (size_t p = 0; p < np && c.subpix; p++) {
                const float want = sub[k][src[p] >= 0 ? (size_t)src[p] : p];
                if (std::memcmp(&got.subpix[k][p], &want, 4) != 0) {
                    CHECK(!"out_sub names the source");
                    break;
                }
            }
            for (long s : src) written += s >= 0;
        }
        CHECK(written > 0);
    }
    // what the wrapper refuses itself, and what the engine refuses through it
    threw = false;
    try {
        weightedMedian(eng, maps, {}, {guides[0]}, &w8, W, H, 2);
    } catch (const Error&) {
        threw = true;
    }
    CHECK(threw);
    threw = false;
    try {
        weightedMedian(eng, maps, {}, guides, nullptr, W, H, 2);
    } catch (const Error&) {
        threw = true;
    }
    CHECK(threw);
    threw = false;
    try {
        weightedMedian(eng, maps, {}, {}, nullptr, W, H, 16);
    } catch (const Error&) {
        threw = true;
    }
    CHECK(threw);
    // ---- the frame: computeArrayDepthSmoothed against the C entry and the
    // stand-alone composition.  The 5x5 rig of test_fill.cpp: 5 px per grid unit,
    // a block of its own in every view
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
            const int x0 = 16 + (int)(rng() % (FW - 44)), y0 = 16 + (int)(rng() % (FH - 44));
            for (int y = y0; y < y0 + 12; y++)
                for (int x = x0; x < x0 + 12; x++)
                    imgs[c][(size_t)y * FW + x] = (uint8_t)(rng() & 255);
        }
        std::vector<ImageView> views;
        for (auto& im : imgs) views.emplace_back(im.data(), FW, FH);
        const double f = cams[12].f;
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
        std::vector<int32_t> vs;
        for (int c = 0; c < 25; c++) {
            vs.push_back(-(c % 5));
            vs.push_back(-(c / 5));
        }
        std::vector<sva_array_pair> ap;
        std::vector<const uint8_t*> ptrs;
        for (auto& v : views) ptrs.push_back(v.data);
        for (const auto& pr : pairs) {
            const PairStep st = pairStep(cams[pr[0]], cams[pr[1]]);
            sva_array_pair a;
            a.ref = pr[0];
            a.other = pr[1];
            a.params = q;
            a.params.dir = st.dir;
            a.params.dir_y = st.dir_y;
            a.baseline = st.baseline;
            ap.push_back(a);
        }
        const int32_t gs[4] = {0, 8, 16, 24};
        const int max_size = 30, max_diff = 1, max_dist = 12, min_found = 3, r = 3;
        for (int select = 0; select < 2; select++) {
            std::vector<double> depth(3 * fnp);
            std::vector<uint16_t> maps(3 * fnp), sup(3 * fnp);
            me.check(sva_array_depth_smoothed(
                me.handle(), ptrs.data(), 25, FW, FH, FW, ap.data(), 24, gs, 3, SVA_ARRAY_GROUPS,
                nullptr, f, ps, 0, SVA_FUSE_MEDIAN, depth.data(), nullptr, nullptr, nullptr,
                maps.data(), nullptr, nullptr, vs.data(), 0, 1, 2, 0, nullptr, nullptr, 1, max_size,
                max_diff, nullptr, max_dist, min_found, SVA_FILL_MEDIAN, nullptr, r, w32.data(), 2,
                select, sup.data()));
            std::vector<std::vector<uint16_t>> mm, ms, fm, m0;
            std::vector<std::vector<uint8_t>> ff;
            auto got = computeArrayDepthSmoothed(me, views, cams, pairs, q, r, &w32, 2, select != 0,
                                                 max_dist, min_found, SVA_FILL_MEDIAN, max_size,
                                                 max_diff, SVA_ARRAY_GROUPS, true, false, 1, 2, 0, 0,
                                                 SVA_FUSE_MEDIAN, 0.05, &mm, &ms);
            CHECK(got.size() == 3 && mm.size() == 3 && ms.size() == 3);
            for (size_t g = 0; g < got.size(); g++) {
                CHECK(got[g].size() == fnp && same_bits(got[g], depth.data() + g * fnp));
                CHECK(same_bits(mm[g], maps.data() + g * fnp));
                CHECK(same_bits(ms[g], sup.data() + g * fnp));
            }
            // the smoothed maps are the filled ones through weightedMedian
            auto filled = computeArrayDepthFilled(me, views, cams, pairs, q, max_dist, min_found,
                                                  SVA_FILL_MEDIAN, max_size, max_diff,
                                                  SVA_ARRAY_GROUPS, true, false, 1, 2, 0, 0,
                                                  SVA_FUSE_MEDIAN, 0.05, &fm, &ff);
            std::vector<ImageView> gv;
            for (int rr : refs) gv.push_back(views[rr]);
            const MedianFiltered alone = weightedMedian(
                eng, fm, {}, gv, &w32, FW, FH, r, 2, true,
                select ? ff : std::vector<std::vector<uint8_t>>{});
            CHECK(alone.maps == mm && alone.support == ms && got != filled && mm != fm);
            // wmed_select with no fill looks at nothing: the filled wrapper's result
            auto a = computeArrayDepthSmoothed(me, views, cams, pairs, q, r, &w32, 2, true, 0,
                                               min_found, SVA_FILL_MEDIAN, max_size, max_diff,
                                               SVA_ARRAY_GROUPS, true, false, 1, 2, 0, 0,
                                               SVA_FUSE_MEDIAN, 0.05, &m0);
            auto b = computeArrayDepthFilled(me, views, cams, pairs, q, 0, min_found,
                                             SVA_FILL_MEDIAN, max_size, max_diff, SVA_ARRAY_GROUPS,
                                             true, false, 1, 2, 0, 0, SVA_FUSE_MEDIAN, 0.05, &fm);
            CHECK(a == b && m0 == fm);
        }
    }
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("wmed mirror ok\n");
    return 0;
}
