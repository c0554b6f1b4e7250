// The C++ mirror of the cross-view check (include/sva.hpp: crossCheck,
// computeArrayDepthChecked) on a GPU.  Built and run by
// tests/test_cross_cpp_gpu.py.  Each of the two calls must equal the C entry
// it wraps, plane for plane.
#include <cmath>
#include <cstdio>
#include <cstring>
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

int main() {
    // the 5x5 rig of CameraStereoVision.cpp:24-39; camera (gx, gy) sees the
    // texture shifted by 5 px per grid unit, and every view has a block of its own
    const int W = 96, H = 80, shift = 5;
    const double ps = 0.036 / W;
    std::vector<Camera> cams;
    for (int y = 0; y < 5; y++)
        for (int x = 0; x < 5; x++)
            cams.emplace_back(0.05, Point3d{-0.1 + x * 0.05, -0.1 + y * 0.05, -0.75}, ps);
    std::mt19937 rng(7);
    const int TW = W + 4 * shift, TH = H + 4 * shift;
    std::vector<uint8_t> tex((size_t)TW * TH);
    for (auto& px : tex) px = (uint8_t)(rng() & 255);
    std::vector<std::vector<uint8_t>> imgs(25, std::vector<uint8_t>((size_t)W * H));
    for (int c = 0; c < 25; c++) {
        const int gx = c % 5 - 2, gy = c / 5 - 2;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++)
                imgs[c][(size_t)y * W + x] =
                    tex[(size_t)(y + (gy + 2) * shift) * TW + x + (gx + 2) * shift];
        const int x0 = 16 + (int)(rng() % (W - 44)), y0 = 16 + (int)(rng() % (H - 44));
        for (int y = y0; y < y0 + 12; y++)
            for (int x = x0; x < x0 + 12; x++) imgs[c][(size_t)y * W + x] = (uint8_t)(rng() & 255);
    }
    std::vector<ImageView> views;
    for (auto& im : imgs) views.emplace_back(im.data(), W, H);
    const double f = cams[12].f;
    const size_t np = (size_t)W * H;

    Engine eng(0);
    MultiEngine me({0}, 2, SVA_MULTI_GATHER_PEER);
    sva_sgm_params q;
    sva_sgm_params_default(&q);
    q.D = 64;

    // three reference cameras, each against its eight neighbours
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

    // ---- the C entry of the frame, by hand ---------------------------------
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
    for (int sub = 0; sub <= 1; sub++) {
        std::vector<double> depth(3 * np);
        std::vector<uint16_t> maps(3 * np);
        std::vector<uint8_t> ag(3 * np), cf(3 * np);
        me.check(sva_array_depth_checked(me.handle(), ptrs.data(), 25, W, H, W, ap.data(), 24, gs, 3,
                                         SVA_ARRAY_GROUPS, nullptr, f, ps, 0, SVA_FUSE_MEDIAN,
                                         depth.data(), nullptr, nullptr, nullptr, maps.data(),
                                         nullptr, nullptr, vs.data(), sub, 1, 2, 0, ag.data(),
                                         cf.data()));
        std::vector<std::vector<uint16_t>> mm;
        std::vector<std::vector<uint8_t>> ma, mc;
        auto got = computeArrayDepthChecked(me, views, cams, pairs, q, SVA_ARRAY_GROUPS, sub != 0, 1,
                                            2, 0, 0, 0.05, &mm, &ma, &mc);
        CHECK(got.size() == 3 && mm.size() == 3 && ma.size() == 3 && mc.size() == 3);
        size_t rejected = 0, agreeing = 0;
        for (size_t g = 0; g < got.size(); g++) {
            CHECK(got[g].size() == np && same_bits(got[g], depth.data() + g * np));
            CHECK(same_bits(mm[g], maps.data() + g * np));
            CHECK(same_bits(ma[g], ag.data() + g * np) && same_bits(mc[g], cf.data() + g * np));
            for (size_t p = 0; p < np; p++) {
                rejected += mm[g][p] == 0xFFFF;
                agreeing += ma[g][p] == 2;
            }
        }
        CHECK(rejected > 0 && rejected < np && agreeing > np);
    }
    // the identity thresholds: computeArrayDepthMulti's result
    {
        std::vector<std::vector<uint16_t>> m0, m1;
        auto a = computeArrayDepthChecked(me, views, cams, pairs, q, SVA_ARRAY_GROUPS, false, 1, 0,
                                          31, 0, 0.05, &m0);
        auto b = computeArrayDepthMulti(me, views, cams, pairs, q, 0, 0.05, &m1);
        CHECK(a == b && m0 == m1);
    }

    // ---- crossCheck against sva_cross_check on the three maps --------------
    {
        std::vector<std::vector<uint16_t>> d;
        std::vector<std::vector<float>> s(3);
        sva_sgm_params qs = q;
        qs.subpixel = 1;
        for (int g = 0; g < 3; g++) {
            std::vector<ImageView> oth;
            std::vector<PairStep> st;
            for (int j = gs[g]; j < gs[g + 1]; j++) {
                oth.push_back(views[pairs[j][1]]);
                st.push_back(pairStep(cams[pairs[j][0]], cams[pairs[j][1]]));
            }
            d.push_back(computeDisparityMulti(eng, views[refs[g]], oth, st, qs, 0, &s[g]));
        }
        std::vector<std::array<int32_t, 2>> step3;
        std::vector<int32_t> flat3;
        std::vector<uint16_t> dd;
        std::vector<float> ss;
        for (int g = 0; g < 3; g++) {
            step3.push_back({vs[2 * refs[g]], vs[2 * refs[g] + 1]});
            flat3.push_back(vs[2 * refs[g]]);
            flat3.push_back(vs[2 * refs[g] + 1]);
            dd.insert(dd.end(), d[g].begin(), d[g].end());
            ss.insert(ss.end(), s[g].begin(), s[g].end());
        }
        std::vector<uint16_t> out(3 * np);
        std::vector<float> out_s(3 * np);
        std::vector<uint8_t> ag(3 * np), cf(3 * np);
        eng.check(sva_cross_check(eng.handle(), dd.data(), ss.data(), 3, W, H, flat3.data(), 0xFFFF,
                                  1, 2, 0, out.data(), out_s.data(), ag.data(), cf.data()));
        const CrossChecked r = crossCheck(eng, d, s, W, H, step3, 1, 2, 0);
        CHECK(r.maps.size() == 3 && r.subpix.size() == 3);
        size_t nan = 0;
        for (size_t g = 0; g < r.maps.size(); g++) {
            CHECK(same_bits(r.maps[g], out.data() + g * np));
            CHECK(same_bits(r.subpix[g], out_s.data() + g * np));
            CHECK(same_bits(r.agree[g], ag.data() + g * np));
            CHECK(same_bits(r.conflict[g], cf.data() + g * np));
            for (size_t p = 0; p < np; p++) {
                const bool rej = r.maps[g][p] == 0xFFFF && d[g][p] != 0xFFFF;
                CHECK(!rej || std::isnan(r.subpix[g][p]));
                nan += rej;
            }
        }
        CHECK(nan > 0);
        const CrossChecked plain = crossCheck(eng, d, {}, W, H, step3, 1, 2, 0);
        CHECK(plain.maps == r.maps && plain.subpix.empty() && plain.agree == r.agree);
    }

    // ---- refusals reach the caller as sva::Error ---------------------------
    int refused = 0;
    try {
        computeArrayDepthChecked(me, views, cams, pairs, q, SVA_ARRAY_PAIRS);
    } catch (const Error& e) {
        refused += e.status == SVA_ERR_UNSUPPORTED;
    }
    try {
        computeArrayDepthChecked(me, views, cams, pairs, q, SVA_ARRAY_GROUPS, false, 1, 32);
    } catch (const Error& e) {
        refused += e.status == SVA_ERR_INVALID_ARG;
    }
    try {
        crossCheck(eng, {std::vector<uint16_t>(np), std::vector<uint16_t>(np)}, {}, W, H,
                   {{0, 0}, {0, 0}});
    } catch (const Error& e) {
        refused += e.status == SVA_ERR_INVALID_ARG;
    }
    CHECK(refused == 3);

    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("cross-check mirror ok\n");
    return 0;
}
