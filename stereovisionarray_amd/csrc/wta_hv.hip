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

// The kernel's geometry argument, from the plan.
WtaHvGeom wta_hv_geom(const AggPlan& p) {
    WtaHvGeom g;
    g.W = p.W; g.H = p.H; g.D = p.D; g.P1 = p.P1; g.P2 = p.P2; g.dmin = p.dmin;
    g.ntx = p.tg.ntx;
    g.nty = p.tg.nty;
    g.nsx = p.tg.nsx;
    g.dreal = p.dreal;
    g.vol = (unsigned)p.vol;
    g.hck = (unsigned)(p.tg.hck_bytes / 2);
    g.vck = (unsigned)(p.tg.vck_bytes / 2);
    g.tiles = g.ntx * g.nty;
    return g;
}

}  // namespace

// (PAIR instances exist only for the D classes whose pair route is enabled,
// minima instances only for those with tune::kPathMinima*; plan_valid has
// refused the others.  A batch: cf's planes hold a plane per frame, like disp
// and sub.)
hipError_t launch_wta_hv(Ctx& c, const AggPlan& p, const AggBuffers& b, uint16_t* disp, float* sub,
                         const ConfOut* cf) {
    DispatchTimer t(c, "wta_hv");
    if (!plan_valid(p) || p.route == AggRoute::Eight || !buffers_fit(p, b) ||
        (cf && (cf->uniqueness < 0 || cf->uniqueness > 100)))
        return hipErrorInvalidValue;
    const WtaHvGeom g = wta_hv_geom(p);
    const dim3 grid((unsigned)(g.tiles * p.frames));
    const uint8_t *L4 = b.volumes, *CK = b.CK, *CKV = b.CKV, *MNP = b.MN;
    t.used = true;
    for_native_d(p.D, [&](auto k) {
        using K = decltype(k);
        with_flag<true>(g.dreal < p.D, [&](auto pad) {
            with_flag<K::kPair>(p.route == AggRoute::Pair, [&](auto pair) {
                with_flag<K::kMinima>(p.minima, [&](auto mn) {
                    constexpr bool PAD = decltype(pad)::value, PAIR = decltype(pair)::value,
                                   MN = decltype(mn)::value;
                    if (cf)   // the confidence instance (the entry point asked for it)
                        hipExtLaunchKernelGGL((wta_hv_conf_kernel<K::DPL, K::kTileLog2, PAD, PAIR, MN>),
                                              grid, dim3(TB), 0, c.stream, t.start, t.stop, 0, b.C,
                                              L4, CK, CKV, MNP, g, disp, sub, *cf);
                    else
                        hipExtLaunchKernelGGL((wta_hv_kernel<K::DPL, K::kTileLog2, PAD, PAIR, MN>),
                                              grid, dim3(TB), 0, c.stream, t.start, t.stop, 0, b.C,
                                              L4, CK, CKV, MNP, g, disp, sub);
                });
            });
        });
    });
    return hipGetLastError();
}

}  // namespace sva
