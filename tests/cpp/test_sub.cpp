// The C++ mirror of the sub-pixel depth entries (include/sva.hpp: fuseDepthSub,
// fuseDepthConfSub, computeArrayDepthSub) on a GPU.  Built and
// run by tests/test_sub_cpp_gpu.py.  Every array route's depth must equal, as
// doubles, what the single-context matcher and the sub-pixel fusion give for
// the same group.
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

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

int main() {
    // the 5x5 rig of CameraStereoVision.cpp:24-39; camera (gx, gy) sees the
    // texture shifted by 5 px per grid unit
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
    }
    std::vector<ImageView> views;
    for (auto& im : imgs) views.emplace_back(im.data(), W, H);
    const double f = cams[12].f;

    Engine eng(0);
    MultiEngine me({0}, 2, SVA_MULTI_GATHER_PEER | SVA_MULTI_GATHER_ALL);
    sva_sgm_params q;
    sva_sgm_params_default(&q);
    q.D = 64;                    // subpixel stays 0: the entry sets it
    sva_sgm_params qs = q;
    qs.subpixel = 1;
    const size_t np = (size_t)W * H;
    const int u = 10;

    // ---- the pair route: 12 against its eight neighbours ------------------
    const auto near8 = getCameraPairs(cams, TO_CENTER_SMALL);
    std::vector<std::vector<uint16_t>> d(8), cmin(8), csec(8);
    std::vector<std::vector<float>> s(8);
    std::vector<double> bl;
    std::vector<ImageView> others8;
    std::vector<PairStep> steps8;
    for (size_t i = 0; i < near8.size(); i++) {
        const PairStep st = pairStep(cams[12], cams[near8[i][1]]);
        sva_sgm_params p = qs;
        p.dir = st.dir;
        p.dir_y = st.dir_y;
        d[i].resize(np);
        s[i].resize(np);
        cmin[i].resize(np);
        csec[i].resize(np);
        eng.check(sva_disparity_sgm_conf(eng.handle(), views[12].data, views[near8[i][1]].data, W,
                                         H, W, &p, u, d[i].data(), s[i].data(), cmin[i].data(),
                                         csec[i].data()));
        bl.push_back(st.baseline);
        others8.push_back(views[near8[i][1]]);
        steps8.push_back(st);
    }
    {
        std::vector<std::vector<uint16_t>> maps;
        auto med = computeArrayDepthSub(me, views, cams, near8, q, SVA_ARRAY_PAIRS, u,
                                        SVA_FUSE_MEDIAN, 0, 0.05, &maps);
        CHECK(med.size() == 1 && maps == d);
        std::vector<uint8_t> nv;
        auto exp = fuseDepthSub(eng, d, s, W, H, bl, f, ps, 0xFFFF, &nv);
        CHECK(same_bits(med[0], exp));
        size_t fractional = 0, counted = 0;
        for (size_t p = 0; p < np; p++) {
            counted += nv[p];
            fractional += !std::isnan(s[0][p]) && s[0][p] != (float)d[0][p];
        }
        CHECK(counted > np && fractional > 0);
        // the integer fusion of the same maps differs somewhere: depth is not quantised
        CHECK(!same_bits(med[0], fuseDepth(eng, d, W, H, bl, f, ps)));
        for (int mode : {SVA_FUSE_MIN_COST, SVA_FUSE_MAX_MARGIN}) {
            auto got = computeArrayDepthSub(me, views, cams, near8, q, SVA_ARRAY_PAIRS, u, mode);
            std::vector<uint8_t> win;
            auto e2 = fuseDepthConfSub(eng, d, s, cmin, csec, W, H, bl, f, ps, mode, 0xFFFF,
                                       nullptr, &win);
            CHECK(same_bits(got[0], e2) && win.size() == np);
        }
        // MIN_COST needs no cost_second
        auto e3 = fuseDepthConfSub(eng, d, s, cmin, {}, W, H, bl, f, ps, SVA_FUSE_MIN_COST);
        CHECK(same_bits(e3, fuseDepthConfSub(eng, d, s, cmin, csec, W, H, bl, f, ps,
                                             SVA_FUSE_MIN_COST)));
    }

    // ---- the multi-baseline route: the same eight pairs in one volume -----
    {
        std::vector<float> sub;
        auto dm = computeDisparityMulti(eng, views[12], others8, steps8, qs, u, &sub);
        std::vector<std::vector<uint16_t>> maps;
        auto got = computeArrayDepthSub(me, views, cams, near8, q, SVA_ARRAY_GROUPS, u,
                                        SVA_FUSE_MEDIAN, 0, 0.05, &maps);
        CHECK(got.size() == 1 && maps.size() == 1 && maps[0] == dm);
        CHECK(same_bits(got[0], fuseDepthSub(eng, {dm}, {sub}, W, H, {bl[0]}, f, ps)));
    }

    // ---- the mixed-baseline route: 12 against all 24, unit = the long baseline
    {
        const auto all24 = getCameraPairs(cams, TO_CENTER);
        std::vector<ImageView> oth;
        std::vector<PairStep> st;
        for (const auto& pr : all24) {
            oth.push_back(views[pr[1]]);
            st.push_back(pairStep(cams[12], cams[pr[1]]));
        }
        std::vector<float> sub;
        auto dm = computeDisparityMixed(eng, views[12], oth, st, 2, qs, u, &sub);
        auto got = computeArrayDepthSub(me, views, cams, all24, q, SVA_ARRAY_GROUPS_MIXED, u);
        CHECK(got.size() == 1);
        CHECK(same_bits(got[0], fuseDepthSub(eng, {dm}, {sub}, W, H, {0.1}, f, ps)));
    }

    // ---- refusals reach the caller as sva::Error --------------------------
    int refused = 0;
    try {
        computeArrayDepthSub(me, views, cams, near8, q, SVA_ARRAY_GROUPS, u, SVA_FUSE_MIN_COST);
    } catch (const Error& e) {
        refused += e.status == SVA_ERR_INVALID_ARG;
    }
    try {
        computeArrayDepthSub(me, views, cams, near8, q, 3);
    } catch (const Error& e) {
        refused += e.status == SVA_ERR_INVALID_ARG;
    }
    try {
        fuseDepthSub(eng, d, {}, W, H, bl, f, ps);
    } catch (const Error& e) {
        refused += e.status == SVA_ERR_INVALID_ARG;
    }
    CHECK(refused == 3);

    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("sub-pixel mirror ok\n");
    return 0;
}
