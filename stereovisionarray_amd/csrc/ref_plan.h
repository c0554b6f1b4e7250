// ref_plan.h -- what refpath.hip launch_ref_match decides before it launches:
// the route, the grid, the shares per tile and the first-minimum keys.  Plain
// C++: no HIP header (tests/test_ref_line_cpu.py compiles it on the host).
#pragma once

#include <cstddef>

#include "sva_tuning.h"

namespace sva {

// largest k of the plane kernel: the ABI maximum.  Region 63 + 2k <= 127
// columns (two per lane) and SAD <= (2k)^2 * 255 < 2^20 for the u32 key.
constexpr int kRefPlaneMaxK = 32;
constexpr int kRefTileCols = 64, kRefTileRows = 32;   // a tile: 4 waves x 8 rows of 64 pixels

// Shares per tile: about four rounds of the chip's workgroup slots in all,
// rounded, within [kPlaneSplitMin, kPlaneSplitMax] -- 1080p (990 tiles, 768
// slots), 1440p and 4K 3, 1280x720 and smaller 6.  Measured with every tile
// split S ways: the shares fill the last round and balance
// the uneven tile work (a Low pair's tiles near the image border carry fewer
// planes); more shares than that pay more per-share setup than they save.
inline int plane_shares(long long tiles, int cu_count) {
    const long long slots = (long long)cu_count * tune::kPlaneMinBlocks;
    if (slots <= 0 || tiles <= 0) return 1;
    long long s = (tune::kPlaneSplitRounds * slots + tiles / 2) / tiles;
    if (s > tune::kPlaneSplitMax) s = tune::kPlaneSplitMax;
    if (s < tune::kPlaneSplitMin) s = tune::kPlaneSplitMin;
    return (int)s;
}

// None: no pixel has a whole window.  Pixel: k > kRefPlaneMaxK, one wave per
// pixel with a u64 wave key.  Plane: the offset-plane kernel, every tile split
// into `shares` workgroups whose per-pixel keys meet in a W x H key buffer.
enum class RefRoute { None, Pixel, Plane };

struct RefMatchPlan {
    RefRoute route;
    int gx, gy;         // Plane: tiles; Pixel: workgroups of 4 pixels x rows
    int shares;         // workgroups per tile; 1: no keys, no finalize pass
    bool wide;          // u64 keys (SAD << 32 | i) instead of u32 (SAD << 12 | i)
    size_t key_size;    // bytes per key
    size_t key_bytes;   // the key buffer the launch needs (0 with one share)
};

// dbg_plane_split (SVA_DEBUG_PLANE_SPLIT, sva_set_debug) 1..16: every tile in
// that many shares, so the parity tests cover every share count at every size.
inline RefMatchPlan ref_match_plan(int W, int H, int k, int cu_count, int dbg_plane_split) {
    RefMatchPlan p{RefRoute::None, 0, 0, 1, false, 0, 0};
    // a line holds at most max(W, H) - 2k + 1 candidates: 4096 or more do not
    // fit the u32 key's 12-bit index field
    p.wide = W >= 4096 || H >= 4096;
    p.key_size = p.wide ? sizeof(unsigned long long) : sizeof(unsigned);
    if (W - 2 * k <= 0 || H - 2 * k <= 0) return p;
    p.route = k > kRefPlaneMaxK ? RefRoute::Pixel : RefRoute::Plane;
    if (p.route == RefRoute::Pixel) {
        p.gx = (W - 2 * k + 3) / 4;
        p.gy = H - 2 * k;
        return p;
    }
    p.gx = (W - 2 * k + kRefTileCols - 1) / kRefTileCols;
    p.gy = (H - 2 * k + kRefTileRows - 1) / kRefTileRows;
    p.shares = plane_shares((long long)p.gx * p.gy, cu_count);
    if (dbg_plane_split >= 1 && dbg_plane_split <= 16) p.shares = dbg_plane_split;
    if (p.shares > 1) p.key_bytes = (size_t)W * H * p.key_size;
    return p;
}

}  // namespace sva
