// agg_plan.h -- one plan for a Mode S aggregation (sgm_paths then wta_hv, or
// sgm_paths alone on eight volumes): the route, the workspace sizes and where
// every plane group starts.  sva_api.cpp plans, sizes and carves through it and
// the two launchers fill their kernel arguments from it; the layout table is
// in DESIGN.md §4.9a.  Plain C++: no HIP header (tests/test_agg_plan_cpu.py
// compiles it into a host program under the sanitizers).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "sva_native_d.h"
#include "sva_tuning.h"

namespace sva {

constexpr int kDiagVolumes = 4;   // [4][H][W][D]: the diagonal directions 4..7
constexpr int kMinimaSeg = 8;     // path minima: bytes (pixels) per segment (§4.17)

// Path minima / the pair route: compiled in for this native D (tune::kPathMinima*,
// tune::kDiagPair*).  A frame with these penalties can take the pair route when
// the u8 pair sum holds 2 * P2.
inline bool path_minima_enabled(int D) {
    bool on = false;
    for_native_d(D, [&](auto k) { on = k.kMinima; });
    return on;
}
inline bool diag_pair_enabled(int D) {
    bool on = false;
    for_native_d(D, [&](auto k) { on = k.kPair; });
    return on;
}
inline bool diag_pair_ok(int D, int P2) { return diag_pair_enabled(D) && 2 * P2 <= 255; }

// Tile pipeline geometry: tiles of 16 columns x seg rows
// (seg = 2^seg_log2), checkpoints every seg columns (horizontal lines) and
// every seg rows (vertical lines).
struct TileGeom {
    int seg_log2;
    int ntx, nty;             // tiles per row / per column (nty = vertical segments)
    int nsx;                  // horizontal segments per row
    size_t hck_bytes;         // [2][H][nsx][D]
    size_t vck_bytes;         // [2][nty][W][D]: directions 2, 3
    size_t hmn_bytes;         // [2][H][nsx][8]: entering minima of directions 0, 1 (§4.17)
    size_t vmn_bytes;         // [2][nty][W][8]: of directions 2, 3
};
inline TileGeom tile_geom(int W, int H, int D) {
    TileGeom t;
    t.seg_log2 = D <= 128 ? tune::kWtahvTileLog2 : tune::kWtahvTileLog2Wide;
    const int seg = 1 << t.seg_log2;
    t.ntx = (W + 15) >> 4;
    t.nty = (H + seg - 1) >> t.seg_log2;
    t.nsx = (W + seg - 1) >> t.seg_log2;
    t.hck_bytes = 2 * (size_t)H * t.nsx * D;
    t.vck_bytes = 2 * (size_t)t.nty * W * D;
    t.hmn_bytes = 2 * (size_t)H * t.nsx * kMinimaSeg;
    t.vmn_bytes = 2 * (size_t)t.nty * W * kMinimaSeg;
    return t;
}

// What is aggregated: `frames` cost volumes [H][W][D] of native width D, of
// which d < dreal are the caller's disparities (0 = D).
struct AggShape {
    int W, H, D;
    int dreal = 0, P1 = 0, P2 = 0, dmin = 0;
};

// Eight: sgm_paths writes all eight L_r volumes and nothing else.  Four: the
// tile pipeline, four diagonal volumes per frame.  Pair: one frame of the tile
// pipeline with two pair-sum volumes (§4.15).
enum class AggRoute { Eight, Four, Pair };

struct AggPlan {
    int W, H, D, dreal, P1, P2, dmin;
    int frames;
    AggRoute route;
    bool minima;              // the minima planes are written and read (§4.17)
    TileGeom tg;
    size_t vol;               // bytes of one [H][W][D] volume
    // The volume workspace holds the frames' volumes back to back from offset
    // 0.  The checkpoint workspace: every frame's horizontal planes, every
    // frame's vertical planes, the pair route's two row-checkpoint planes,
    // the minima planes (horizontal, then vertical).
    size_t paths_bytes, ckpt_bytes;
    size_t hck_off, vck_off, pair_off, mn_off;
    // frame f of a batch: C + f * c_stride, volumes + f * vol_stride,
    // hck_off + f * hck_stride, vck_off + f * vck_stride
    size_t c_stride, vol_stride, hck_stride, vck_stride;
};

inline AggPlan agg_plan(const AggShape& s, int frames, AggRoute route, bool minima) {
    AggPlan p;
    p.W = s.W; p.H = s.H; p.D = s.D; p.P1 = s.P1; p.P2 = s.P2; p.dmin = s.dmin;
    p.dreal = s.dreal > 0 && s.dreal < s.D ? s.dreal : s.D;
    p.frames = frames;
    p.route = route;
    p.minima = minima;
    p.tg = tile_geom(s.W, s.H, s.D);
    p.vol = (size_t)s.W * s.H * (size_t)s.D;
    const bool tile = route != AggRoute::Eight;
    const size_t n = (size_t)frames;
    p.paths_bytes = p.vol * n * (route == AggRoute::Eight ? 8 : route == AggRoute::Pair ? 2 : kDiagVolumes);
    p.hck_off = 0;
    p.vck_off = tile ? p.tg.hck_bytes * n : 0;
    p.pair_off = tile ? p.vck_off + p.tg.vck_bytes * n : 0;
    // (one row-checkpoint plane per diagonal pair: [2][nty][W][D] again; every
    // term so far is a multiple of D, so the minima planes are 8-byte aligned)
    p.mn_off = p.pair_off + (route == AggRoute::Pair ? p.tg.vck_bytes : 0);
    p.ckpt_bytes = p.mn_off + (minima ? p.tg.hmn_bytes + p.tg.vmn_bytes : 0);
    p.c_stride = p.vol;
    p.vol_stride = kDiagVolumes * p.vol;
    p.hck_stride = p.tg.hck_bytes;
    p.vck_stride = p.tg.vck_bytes;
    return p;
}

// A frame on the context's workspaces: the pair route where
// this D has it, the pair sums fit a u8 and the frame has pair_min_pixels
// pixels, so that the pair waves' chain is not the bound (the caller passes
// tune::kDiagPairMinPixels or its debug override); else four volumes.  Minima
// planes wherever this D has them.
inline AggPlan frame_plan(const AggShape& s, long long pair_min_pixels) {
    const bool pair = diag_pair_ok(s.D, s.P2) && (long long)s.W * s.H >= pair_min_pixels;
    return agg_plan(s, 1, pair ? AggRoute::Pair : AggRoute::Four, path_minima_enabled(s.D));
}
// m frames of one shape in one launch of each kernel.
inline AggPlan batch_plan(const AggShape& s, int m) { return agg_plan(s, m, AggRoute::Four, false); }
// sva_paths_tile_d / sva_wta_hv_d: the caller's own buffers, one per plane
// group (tg.hck_bytes, tg.vck_bytes), so the offsets are not used.
inline AggPlan stage_plan(const AggShape& s) { return agg_plan(s, 1, AggRoute::Four, false); }
// sva_paths_d / sva_aggregate_d.
inline AggPlan eight_plan(const AggShape& s) { return agg_plan(s, 1, AggRoute::Eight, false); }

// The legality rules of a launch: a native D with 32-bit volume offsets; a
// batch only on four volumes; the pair route and the minima planes only for
// one frame of the tile pipeline whose D class has them, the pair sums in a u8
// and the minima in 8-pixel segments.
inline bool plan_valid(const AggPlan& p) {
    int tile_log2 = -1;
    if (!for_native_d(p.D, [&](auto k) { tile_log2 = k.kTileLog2; })) return false;
    if (p.W <= 0 || p.H <= 0 || p.frames < 1 || p.vol >= (size_t)1 << 32) return false;
    if (p.route == AggRoute::Eight) return p.frames == 1 && !p.minima;
    if (p.tg.seg_log2 != tile_log2) return false;
    if (p.route == AggRoute::Pair && (p.frames != 1 || !diag_pair_ok(p.D, p.P2))) return false;
    if (p.minima && (p.frames != 1 || !path_minima_enabled(p.D) || (1 << p.tg.seg_log2) != kMinimaSeg))
        return false;
    return true;
}

// Workspace sizes that hold every frame_plan of this shape, whatever its
// penalties and pixel threshold (sva_reserve; any D > 0: a D with no native
// class has neither the pair route nor minima).
struct AggReserve {
    size_t paths_bytes, ckpt_bytes;
};
inline AggReserve reserve_plan(int W, int H, int D) {
    const AggShape s{W, H, D};
    const bool mn = path_minima_enabled(D);
    const AggPlan four = agg_plan(s, 1, AggRoute::Four, mn);
    const AggPlan pair = agg_plan(s, 1, diag_pair_enabled(D) ? AggRoute::Pair : AggRoute::Four, mn);
    return {std::max(four.paths_bytes, pair.paths_bytes), std::max(four.ckpt_bytes, pair.ckpt_bytes)};
}

// The device buffers of one launch pair.  volumes: the plan's route volumes.
// CK: the horizontal checkpoints; CKV: the vertical ones, followed on the pair
// route by its two row-checkpoint planes; MN: the minima planes, null without.
struct AggBuffers {
    const uint8_t* C = nullptr;
    uint8_t* volumes = nullptr;
    uint8_t *CK = nullptr, *CKV = nullptr, *MN = nullptr;
};
// The plan's buffers inside a context's two allocations, and the cost volume(s) C.
inline AggBuffers carve(const AggPlan& p, const uint8_t* C, void* paths, void* ckpt) {
    AggBuffers b;
    b.C = C;
    b.volumes = (uint8_t*)paths;
    if (p.route != AggRoute::Eight) {
        b.CK = (uint8_t*)ckpt + p.hck_off;
        b.CKV = (uint8_t*)ckpt + p.vck_off;
        if (p.minima) b.MN = (uint8_t*)ckpt + p.mn_off;
    }
    return b;
}
// Every buffer the plan's kernels touch is there.
inline bool buffers_fit(const AggPlan& p, const AggBuffers& b) {
    const bool tile = p.route != AggRoute::Eight;
    return (b.CK != nullptr) == tile && (b.CKV != nullptr) == tile && (b.MN != nullptr) == p.minima;
}

}  // namespace sva
