// wta_hv.hip -- the tile pipeline's final kernel (SURVEY.md
// §8a rows A12-A13): horizontal AND vertical path recompute + path sum + WTA
// (+ sub-pixel) per 16 x TY pixel tile.
//
// sgm_paths in tile mode (ckpt 2) leaves four u8 volumes (the diagonal
// directions) and checkpoints every TY pixels: the horizontal lines' L state
// at the last / first column of every TY-column segment, the vertical lines'
// at the last / first row of every TY-row segment.  One 256-thread workgroup
// owns one tile of 16 columns x TY rows, with the path kernel's lane layout
// (lane k of a 16-lane DPP row owns disparities [k*DPL, k*DPL + DPL)):
//   phase V  row-slot s runs column x0 + s: the downward recurrence over the
//            tile's rows from the checkpoint above the tile, and the upward
//            one from the checkpoint below it; V = L_2 + L_3 of every pixel
//            goes to LDS (u16 pairs).
//   phase H  row-slot s runs one TY-pixel row segment (16 / TY per tile row):
//            left-to-right from the checkpoint left of it (L_0 kept in
//            registers, u16 pairs), then right-to-left from the one right of
//            it; at each pixel S = L_1 + L_0 + V + the four diagonal volumes,
//            and the first-minimum WTA (+ parabola) picks d*.
// Every recurrence restarts from the exact state the path kernel had, so L,
// S, d* and the sub-pixel value are bit-identical to the 8-volume route.
// On the frame route of the D classes with tune::kPathMinima* every step's m
// is read from the path kernel's minima planes as well.
//
// Bytes per disparity: 1 C read (phase H re-reads the tile's cost words from
// L2, where phase V just brought them) + 4 volume reads, and the path kernel
// writes 4 volumes instead of 6: -4 B/disp against the wta_h route (§4.6).
#include "sgm_common.h"
#include "wta_common.h"
#include "sva_tuning.h"

namespace sva {
namespace {

using namespace sgm;

constexpr int TB = 256;             // 16 slots of 16 lanes
constexpr int TW = 16;              // tile columns

struct WtaHvGeom {
    int W, H, D, P1, P2, dmin;
    int ntx, nty;     // tiles per row / per column
    int nsx;          // horizontal checkpoint segments per row, ceil(W / TY)
    int dreal;        // disparities of the caller (< D: padded frame)
    unsigned vol;     // bytes of one [H][W][D] volume (< 2^32)
    unsigned hck;     // bytes of one horizontal checkpoint plane [H][nsx][D]
    unsigned vck;     // bytes of one vertical checkpoint plane [nty][W][D]
    int tiles;        // tiles per frame, ntx * nty (a batch: frame = block / tiles)
};

// Prefetch depth (pixels) of the diagonal volumes in the last pass.
template <int DPL, bool PAIR> constexpr int pf_vol() {
    return PAIR ? tune::kWtahvPfVolPair : DPL >= 16 ? tune::kWtahvPfVol16 : DPL <= 4 ? tune::kWtahvPfVol4 : tune::kWtahvPfVol;
}

// PAIR (the pair route): L4 holds two pair-sum volumes
// E = (L_a - C) + (L_b - C) for the diagonal pairs 4+5 and 6+7 instead of four
// L_r volumes; the missing 4C enters V in phase V.
// MN (path minima): every step of phase V and phase H takes
// its m from the planes the path kernel wrote (MNP: [2][H][nsx][8], then
// [2][nty][W][8]; byte i of a segment = step i of the recurrence, in both
// directions) instead of reducing the state it just formed: the only row
// minimum left is the WTA's.
// The kernel's text is wta_hv_tile.inc: wta_hv_kernel, and its confidence
// instance wta_hv_conf_kernel (cost_min / cost_second planes
// and the uniqueness filter, a ConfOut argument after `sub`).
#define SVA_WTAHV_CONF 0
#include "wta_hv_tile.inc"
#undef SVA_WTAHV_CONF
#define SVA_WTAHV_CONF 1
#include "wta_hv_tile.inc"
#undef SVA_WTAHV_CONF

// (PAIR instances exist only for the D classes whose pair route is enabled,
// minima instances only for those with tune::kPathMinima*; launch_wta_hv has
// refused pair = true or a minima plane for the others)
template <int DPL, int TYL, bool PAIR, bool MN>
void wtahv_launch_mn(bool pad, dim3 grid, hipStream_t s, hipEvent_t start, hipEvent_t stop,
                     const uint8_t* C, const uint8_t* L4, const uint8_t* CK, const uint8_t* CKV,
                     const uint8_t* MNP, const WtaHvGeom& g, uint16_t* disp, float* sub,
                     const ConfOut* cf) {
    if (cf) {   // the confidence instance (the entry point asked for it)
        if (pad)
            hipExtLaunchKernelGGL((wta_hv_conf_kernel<DPL, TYL, true, PAIR, MN>), grid, dim3(TB), 0,
                                  s, start, stop, 0, C, L4, CK, CKV, MNP, g, disp, sub, *cf);
        else
            hipExtLaunchKernelGGL((wta_hv_conf_kernel<DPL, TYL, false, PAIR, MN>), grid, dim3(TB), 0,
                                  s, start, stop, 0, C, L4, CK, CKV, MNP, g, disp, sub, *cf);
        return;
    }
    if (pad)
        hipExtLaunchKernelGGL((wta_hv_kernel<DPL, TYL, true, PAIR, MN>), grid, dim3(TB), 0, s, start,
                              stop, 0, C, L4, CK, CKV, MNP, g, disp, sub);
    else
        hipExtLaunchKernelGGL((wta_hv_kernel<DPL, TYL, false, PAIR, MN>), grid, dim3(TB), 0, s, start,
                              stop, 0, C, L4, CK, CKV, MNP, g, disp, sub);
}
template <int DPL, int TYL, bool PAIR, bool MNEN>
void wtahv_launch(bool pad, dim3 grid, hipStream_t s, hipEvent_t start, hipEvent_t stop,
                  const uint8_t* C, const uint8_t* L4, const uint8_t* CK, const uint8_t* CKV,
                  const uint8_t* MNP, const WtaHvGeom& g, uint16_t* disp, float* sub,
                  const ConfOut* cf) {
    if constexpr (MNEN) {
        if (MNP) {
            wtahv_launch_mn<DPL, TYL, PAIR, true>(pad, grid, s, start, stop, C, L4, CK, CKV, MNP, g,
                                                  disp, sub, cf);
            return;
        }
    }
    wtahv_launch_mn<DPL, TYL, PAIR, false>(pad, grid, s, start, stop, C, L4, CK, CKV, nullptr, g,
                                           disp, sub, cf);
}

}  // namespace

bool wta_hv_supported(int D) { return D == 64 || D == 128 || D == 192 || D == 256; }

hipError_t launch_wta_hv(Ctx& c, const uint8_t* C, const uint8_t* L4, const uint8_t* CK,
                         const uint8_t* CKV, int W, int H, int D, int P1, int P2, int dmin,
                         uint16_t* disp, float* sub, int dreal, int npair, bool pair,
                         const uint8_t* MN, const ConfOut* cf) {
    DispatchTimer t(c, "wta_hv");
    if (!wta_hv_supported(D)) return hipErrorInvalidValue;
    const TileGeom tg = tile_geom(W, H, D);
    WtaHvGeom g;
    g.W = W; g.H = H; g.D = D; g.P1 = P1; g.P2 = P2; g.dmin = dmin;
    g.dreal = dreal > 0 && dreal < D ? dreal : D;
    g.ntx = tg.ntx;
    g.nty = tg.nty;
    g.nsx = tg.nsx;
    const size_t vol = (size_t)W * H * D;
    if (vol >= (size_t)1 << 32) return hipErrorInvalidValue;
    g.vol = (unsigned)vol;
    g.hck = (unsigned)(tg.hck_bytes / 2);
    g.vck = (unsigned)(tg.vck_bytes / 2);
    const bool pad = g.dreal < D;
    if (npair < 1) return hipErrorInvalidValue;
    // (a batch, npair > 1: cf's planes hold npair frames, like disp and sub)
    if (cf && (cf->uniqueness < 0 || cf->uniqueness > 100)) return hipErrorInvalidValue;
    g.tiles = g.ntx * g.nty;
    const dim3 grid((unsigned)(g.tiles * npair));
#define SVA_WTAHV(DPL_, TYL_, MN_)                                                            \
    wtahv_launch<DPL_, TYL_, false, (MN_) != 0>(pad, grid, c.stream, t.start, t.stop, C, L4,  \
                                                CK, CKV, MN, g, disp, sub, cf);               \
    t.used = true
#define SVA_WTAHV_P(DPL_, TYL_, EN_, MN_)                                                     \
    if (pair) {                                                                               \
        wtahv_launch<DPL_, TYL_, (EN_) != 0, (MN_) != 0>(pad, grid, c.stream, t.start,        \
                                                         t.stop, C, L4, CK, CKV, MN, g, disp, \
                                                         sub, cf);                            \
        t.used = true;                                                                        \
    } else {                                                                                  \
        SVA_WTAHV(DPL_, TYL_, MN_);                                                           \
    }
    constexpr int TYL = tune::kWtahvTileLog2, TYLW = tune::kWtahvTileLog2Wide;
    if (tg.seg_log2 != (D <= 128 ? TYL : TYLW)) return hipErrorInvalidValue;
    if (pair && (npair != 1 || !diag_pair_ok(D, P2))) return hipErrorInvalidValue;
    if (MN && (npair != 1 || !path_minima_enabled(D) || (1 << tg.seg_log2) != sgm::kMinimaSeg))
        return hipErrorInvalidValue;
    switch (D) {
        case 64: SVA_WTAHV_P(4, TYL, tune::kDiagPair4, tune::kPathMinima4); break;
        case 128: SVA_WTAHV_P(8, TYL, tune::kDiagPair8, tune::kPathMinima8); break;
        case 192: SVA_WTAHV_P(12, TYLW, tune::kDiagPair12, tune::kPathMinima12); break;
        case 256: SVA_WTAHV_P(16, TYLW, tune::kDiagPair16, tune::kPathMinima16); break;
        default: return hipErrorInvalidValue;
    }
#undef SVA_WTAHV_P
#undef SVA_WTAHV
    return hipGetLastError();
}

}  // namespace sva
