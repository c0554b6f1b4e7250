// The C++ mirror of hole filling (include/sva.hpp: fillHoles,
// computeArrayDepthFilled) on a GPU.  Built and run by
// tests/test_fill_cpp_gpu.py.  Each call must equal the C entry it wraps, plane
// for plane; fillHoles is also held to a ray walk written here.
#include <algorithm>
#include <array>
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

// One map by the rule, ray by ray: out, n_found and the source index (-1: not filled).
static void walk(const std::vector<uint16_t>& d, int W, int H, int max_dist, int min_found, int mode,
                 std::vector<uint16_t>& out, std::vector<uint8_t>& found, std::vector<long>& src) {
    static const int DX[8] = {1, -1, 0, 0, 1, -1, -1, 1}, DY[8] = {0, 0, 1, -1, 1, -1, 1, -1};
    auto ok = [&](size_t p) { return d[p] != 0xFFFF && d[p] != 0; };
    out = d;
    found.assign(d.size(), 0);
    src.assign(d.size(), -1);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * W + x;
            if (ok(p)) continue;
            std::vector<std::tuple<int, int, int, long>> c;
            for (int k = 0; k < 8; k++)
                for (int j = 1; j <= max_dist; j++) {
                    const int qx = x + j * DX[k], qy = y + j * DY[k];
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) break;
                    const size_t q = (size_t)qy * W + qx;
                    if (ok(q)) {
                        c.emplace_back((int)d[q], j, k, (long)q);
                        break;
                    }
                }
            std::sort(c.begin(), c.end());
            const int n = (int)c.size();
            found[p] = (uint8_t)n;
            if (n < min_found || n < 1) continue;
            const int e = mode == SVA_FILL_MIN ? 0 : mode == SVA_FILL_SECOND ? std::min(1, n - 1)
                                                                             : (n - 1) / 2;
            out[p] = (uint16_t)std::get<0>(c[e]);
            src[p] = std::get<3>(c[e]);
        }
}

int main() {
    // the 5x5 rig of test_speckle.cpp: 5 px per grid unit, a block of its own in every view
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
    const int max_size = 30, max_diff = 1, max_dist = 12, min_found = 3;

    // ---- the group frame, with the check: the wrapper against the C entry ----
    std::vector<std::vector<uint16_t>> filtered_maps;
    for (int mode = SVA_FILL_MIN; mode <= SVA_FILL_MEDIAN; mode++) {
        std::vector<double> depth(3 * np);
        std::vector<uint16_t> maps(3 * np);
        std::vector<uint8_t> found(3 * np);
        me.check(sva_array_depth_filled(me.handle(), ptrs.data(), 25, W, H, W, ap.data(), 24, gs, 3,
                                        SVA_ARRAY_GROUPS, nullptr, f, ps, 0, SVA_FUSE_MEDIAN,
                                        depth.data(), nullptr, nullptr, nullptr, maps.data(), nullptr,
                                        nullptr, vs.data(), 0, 1, 2, 0, nullptr, nullptr, 1, max_size,
                                        max_diff, nullptr, max_dist, min_found, mode, found.data()));
        std::vector<std::vector<uint16_t>> mm, m0, m1;
        std::vector<std::vector<uint8_t>> mf;
        auto got = computeArrayDepthFilled(me, views, cams, pairs, q, max_dist, min_found, mode,
                                           max_size, max_diff, SVA_ARRAY_GROUPS, true, false, 1, 2, 0,
                                           0, SVA_FUSE_MEDIAN, 0.05, &mm, &mf);
        CHECK(got.size() == 3 && mm.size() == 3 && mf.size() == 3);
        for (size_t g = 0; g < got.size(); g++) {
            CHECK(got[g].size() == np && same_bits(got[g], depth.data() + g * np));
            CHECK(same_bits(mm[g], maps.data() + g * np) && same_bits(mf[g], found.data() + g * np));
        }
        // max_dist 0: the filtered wrapper's result
        auto a = computeArrayDepthFilled(me, views, cams, pairs, q, 0, min_found, mode, max_size,
                                         max_diff, SVA_ARRAY_GROUPS, true, false, 1, 2, 0, 0,
                                         SVA_FUSE_MEDIAN, 0.05, &m0);
        auto b = computeArrayDepthFiltered(me, views, cams, pairs, q, max_size, max_diff,
                                           SVA_ARRAY_GROUPS, true, false, 1, 2, 0, 0, SVA_FUSE_MEDIAN,
                                           0.05, &m1);
        CHECK(a == b && m0 == m1 && got != b);
        // the filled maps are the filtered ones through fillHoles, and the rule's
        const HolesFilled r = fillHoles(eng, m1, {}, W, H, max_dist, min_found, mode);
        CHECK(r.maps == mm && r.n_found == mf && r.subpix.empty());
        size_t filled = 0;
        for (size_t g = 0; g < 3; g++) {
            std::vector<uint16_t> out;
            std::vector<uint8_t> nf;
            std::vector<long> src;
            walk(m1[g], W, H, max_dist, min_found, mode, out, nf, src);
            CHECK(r.maps[g] == out && r.n_found[g] == nf);
            for (long s : src) filled += s >= 0;
        }
        CHECK(filled > 0);
        filtered_maps = m1;
    }

    // ---- the pair frame: every pair's map, in `pairs` order -----------------
    {
        std::vector<std::vector<uint16_t>> mm, m1;
        std::vector<std::vector<uint8_t>> mf;
        auto got = computeArrayDepthFilled(me, views, cams, pairs, q, max_dist, min_found,
                                           SVA_FILL_SECOND, max_size, max_diff, SVA_ARRAY_PAIRS, false,
                                           false, 1, 1, 0, 0, SVA_FUSE_MEDIAN, 0.05, &mm, &mf);
        auto plain = computeArrayDepthFiltered(me, views, cams, pairs, q, max_size, max_diff,
                                               SVA_ARRAY_PAIRS, false, false, 1, 1, 0, 0,
                                               SVA_FUSE_MEDIAN, 0.05, &m1);
        CHECK(got.size() == plain.size() && mm.size() == pairs.size() && mf.size() == pairs.size());
        const HolesFilled r = fillHoles(eng, m1, {}, W, H, max_dist, min_found, SVA_FILL_SECOND);
        CHECK(r.maps == mm && r.n_found == mf);
        CHECK(got != plain);
    }

    // ---- fillHoles with sub-pixel maps against sva_fill_holes and the walk ---
    {
        std::vector<std::vector<float>> s(3);
        std::vector<uint16_t> dd;
        std::vector<float> ss;
        for (int g = 0; g < 3; g++) {
            s[g].resize(np);
            for (size_t p = 0; p < np; p++) s[g][p] = (float)p + 0.25f;   // names its pixel
            dd.insert(dd.end(), filtered_maps[g].begin(), filtered_maps[g].end());
            ss.insert(ss.end(), s[g].begin(), s[g].end());
        }
        std::vector<uint16_t> out(3 * np);
        std::vector<float> out_s(3 * np);
        std::vector<uint8_t> found(3 * np);
        eng.check(sva_fill_holes(eng.handle(), dd.data(), ss.data(), 3, W, H, 0xFFFF, max_dist, 1,
                                 SVA_FILL_MEDIAN, out.data(), out_s.data(), found.data()));
        const HolesFilled r = fillHoles(eng, filtered_maps, s, W, H, max_dist, 1, SVA_FILL_MEDIAN);
        CHECK(r.maps.size() == 3 && r.subpix.size() == 3);
        size_t moved = 0;
        for (size_t g = 0; g < 3; g++) {
            CHECK(same_bits(r.maps[g], out.data() + g * np));
            CHECK(same_bits(r.subpix[g], out_s.data() + g * np));
            CHECK(same_bits(r.n_found[g], found.data() + g * np));
            std::vector<uint16_t> wo;
            std::vector<uint8_t> wf;
            std::vector<long> src;
            walk(filtered_maps[g], W, H, max_dist, 1, SVA_FILL_MEDIAN, wo, wf, src);
            for (size_t p = 0; p < np; p++) {
                CHECK(r.subpix[g][p] == s[g][src[p] >= 0 ? (size_t)src[p] : p]);
                moved += src[p] >= 0;
            }
        }
        CHECK(moved > 0);
        const HolesFilled same = fillHoles(eng, filtered_maps, s, W, H, 0);
        CHECK(same.maps == filtered_maps && same.subpix == s);
    }

    // ---- refusals reach the caller as sva::Error ---------------------------
    int refused = 0;
    try {
        computeArrayDepthFilled(me, views, cams, pairs, q, 256);
    } catch (const Error& e) {
        refused += e.status == SVA_ERR_INVALID_ARG;
    }
    try {
        computeArrayDepthFilled(me, views, cams, pairs, q, 8, 9);
    } catch (const Error& e) {
        refused += e.status == SVA_ERR_INVALID_ARG;
    }
    try {
        fillHoles(eng, {std::vector<uint16_t>(np)}, {}, W, H, 5, 1, 3);
    } catch (const Error& e) {
        refused += e.status == SVA_ERR_INVALID_ARG;
    }
    try {
        fillHoles(eng, {std::vector<uint16_t>(np)}, {std::vector<float>(np), std::vector<float>(np)}, W,
                  H, 5);
    } catch (const Error& e) {
        refused += e.status == SVA_ERR_INVALID_ARG;
    }
    CHECK(refused == 4);

    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("fill mirror ok\n");
    return 0;
}
