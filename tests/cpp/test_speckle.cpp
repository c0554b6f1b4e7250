// The C++ mirror of the speckle filter (include/sva.hpp: filterSpeckles,
// computeArrayDepthFiltered) on a GPU.  Built and run by
// tests/test_speckle_cpp_gpu.py.  Each call must equal the C entry it wraps,
// plane for plane; filterSpeckles is also held to a flood fill written here.
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

// comp_size of one map by flood fill.
static std::vector<uint32_t> flood(const std::vector<uint16_t>& d, int W, int H, int max_diff) {
    auto ok = [&](size_t p) { return d[p] != 0xFFFF && d[p] != 0; };
    std::vector<uint32_t> size(d.size(), 0);
    std::vector<char> seen(d.size(), 0);
    for (size_t seed = 0; seed < d.size(); seed++) {
        if (seen[seed] || !ok(seed)) continue;
        std::vector<size_t> stack{seed}, members;
        seen[seed] = 1;
        while (!stack.empty()) {
            const size_t p = stack.back();
            stack.pop_back();
            members.push_back(p);
            const int x = (int)(p % W), y = (int)(p / W);
            const int nx[4] = {x + 1, x - 1, x, x}, ny[4] = {y, y, y + 1, y - 1};
            for (int k = 0; k < 4; k++) {
                if (nx[k] < 0 || nx[k] >= W || ny[k] < 0 || ny[k] >= H) continue;
                const size_t q = (size_t)ny[k] * W + nx[k];
                if (seen[q] || !ok(q) || std::abs((int)d[p] - (int)d[q]) > max_diff) continue;
                seen[q] = 1;
                stack.push_back(q);
            }
        }
        for (size_t p : members) size[p] = (uint32_t)members.size();
    }
    return size;
}

int main() {
    // the 5x5 rig of test_cross.cpp: 5 px per grid unit, a block of its own in every view
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
    const int max_size = 30, max_diff = 1;

    // ---- the group frame, with and without the check ------------------------
    std::vector<std::vector<uint16_t>> checked_maps;
    for (int check = 0; check <= 1; check++) {
        std::vector<double> depth(3 * np);
        std::vector<uint16_t> maps(3 * np);
        std::vector<uint32_t> size(3 * np);
        me.check(sva_array_depth_filtered(me.handle(), ptrs.data(), 25, W, H, W, ap.data(), 24, gs, 3,
                                          SVA_ARRAY_GROUPS, nullptr, f, ps, 0, SVA_FUSE_MEDIAN,
                                          depth.data(), nullptr, nullptr, nullptr, maps.data(),
                                          nullptr, nullptr, vs.data(), 0, 1, 2, 0, nullptr, nullptr,
                                          check, max_size, max_diff, size.data()));
        std::vector<std::vector<uint16_t>> mm;
        std::vector<std::vector<uint32_t>> ms;
        auto got = computeArrayDepthFiltered(me, views, cams, pairs, q, max_size, max_diff,
                                             SVA_ARRAY_GROUPS, check != 0, false, 1, 2, 0, 0,
                                             SVA_FUSE_MEDIAN, 0.05, &mm, &ms);
        CHECK(got.size() == 3 && mm.size() == 3 && ms.size() == 3);
        for (size_t g = 0; g < got.size(); g++) {
            CHECK(got[g].size() == np && same_bits(got[g], depth.data() + g * np));
            CHECK(same_bits(mm[g], maps.data() + g * np) && same_bits(ms[g], size.data() + g * np));
        }
        // max_size 0: the unfiltered wrapper's result
        std::vector<std::vector<uint16_t>> m0, m1;
        auto a = computeArrayDepthFiltered(me, views, cams, pairs, q, 0, max_diff, SVA_ARRAY_GROUPS,
                                           check != 0, false, 1, 2, 0, 0, SVA_FUSE_MEDIAN, 0.05, &m0);
        auto b = check ? computeArrayDepthChecked(me, views, cams, pairs, q, SVA_ARRAY_GROUPS, false,
                                                  1, 2, 0, 0, 0.05, &m1)
                       : computeArrayDepthMulti(me, views, cams, pairs, q, 0, 0.05, &m1);
        CHECK(a == b && m0 == m1);
        // the filtered maps are the unfiltered ones through filterSpeckles
        const SpeckleFiltered r = filterSpeckles(eng, m1, {}, W, H, max_size, max_diff);
        CHECK(r.maps == mm && r.comp_size == ms && r.subpix.empty());
        size_t removed = 0;
        for (size_t g = 0; g < 3; g++) {
            CHECK(r.comp_size[g] == flood(m1[g], W, H, max_diff));
            for (size_t p = 0; p < np; p++) {
                const bool gone = r.comp_size[g][p] != 0 && r.comp_size[g][p] <= (uint32_t)max_size;
                CHECK(r.maps[g][p] == (gone ? 0xFFFF : m1[g][p]));
                removed += gone;
            }
        }
        CHECK(removed > 0 && removed < np);
        if (check) checked_maps = m1;
    }

    // ---- the pair frame: every pair's map, in `pairs` order -----------------
    {
        std::vector<std::vector<uint16_t>> mm, m1;
        std::vector<std::vector<uint32_t>> ms;
        auto got = computeArrayDepthFiltered(me, views, cams, pairs, q, max_size, max_diff,
                                             SVA_ARRAY_PAIRS, false, false, 1, 1, 0, 0,
                                             SVA_FUSE_MIN_COST, 0.05, &mm, &ms);
        auto plain = computeArrayDepthConf(me, views, cams, pairs, q, 0, SVA_FUSE_MIN_COST, 0.05, &m1);
        CHECK(got.size() == plain.size() && mm.size() == pairs.size() && ms.size() == pairs.size());
        const SpeckleFiltered r = filterSpeckles(eng, m1, {}, W, H, max_size, max_diff);
        CHECK(r.maps == mm && r.comp_size == ms);
        CHECK(got != plain);
    }

    // ---- filterSpeckles with sub-pixel maps against sva_filter_speckles -----
    {
        std::vector<std::vector<float>> s(3);
        std::vector<uint16_t> dd;
        std::vector<float> ss;
        for (int g = 0; g < 3; g++) {
            s[g].resize(np);
            for (size_t p = 0; p < np; p++) s[g][p] = (float)checked_maps[g][p] + 0.25f;
            dd.insert(dd.end(), checked_maps[g].begin(), checked_maps[g].end());
            ss.insert(ss.end(), s[g].begin(), s[g].end());
        }
        std::vector<uint16_t> out(3 * np);
        std::vector<float> out_s(3 * np);
        std::vector<uint32_t> size(3 * np);
        eng.check(sva_filter_speckles(eng.handle(), dd.data(), ss.data(), 3, W, H, 0xFFFF, max_size,
                                      max_diff, out.data(), out_s.data(), size.data()));
        const SpeckleFiltered r = filterSpeckles(eng, checked_maps, s, W, H, max_size, max_diff);
        CHECK(r.maps.size() == 3 && r.subpix.size() == 3);
        size_t nan = 0;
        for (size_t g = 0; g < 3; g++) {
            CHECK(same_bits(r.maps[g], out.data() + g * np));
            CHECK(same_bits(r.subpix[g], out_s.data() + g * np));
            CHECK(same_bits(r.comp_size[g], size.data() + g * np));
            for (size_t p = 0; p < np; p++) {
                const bool gone = r.maps[g][p] == 0xFFFF && checked_maps[g][p] != 0xFFFF;
                CHECK(gone == (bool)std::isnan(r.subpix[g][p]));
                nan += gone;
            }
        }
        CHECK(nan > 0);
        const SpeckleFiltered same = filterSpeckles(eng, checked_maps, s, W, H, 0, max_diff);
        CHECK(same.maps == checked_maps && same.subpix == s);
    }

    // ---- refusals reach the caller as sva::Error ---------------------------
    int refused = 0;
    try {
        computeArrayDepthFiltered(me, views, cams, pairs, q, max_size, max_diff, SVA_ARRAY_PAIRS, true);
    } catch (const Error& e) {
        refused += e.status == SVA_ERR_UNSUPPORTED;
    }
    try {
        computeArrayDepthFiltered(me, views, cams, pairs, q, -1, max_diff);
    } catch (const Error& e) {
        refused += e.status == SVA_ERR_INVALID_ARG;
    }
    try {
        filterSpeckles(eng, {std::vector<uint16_t>(np)}, {}, W, H, 5, -1);
    } catch (const Error& e) {
        refused += e.status == SVA_ERR_INVALID_ARG;
    }
    try {
        filterSpeckles(eng, {std::vector<uint16_t>(np)}, {std::vector<float>(np), std::vector<float>(np)},
                       W, H, 5, 1);
    } catch (const Error& e) {
        refused += e.status == SVA_ERR_INVALID_ARG;
    }
    CHECK(refused == 4);

    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("speckle mirror ok\n");
    return 0;
}
