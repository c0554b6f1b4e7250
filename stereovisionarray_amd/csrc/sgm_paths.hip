// sgm_paths.hip -- 8-direction SGM path aggregation (DESIGN.md §2.3 / §4.3,
// SURVEY.md §8a row A12).  All eight directions run in ONE launch.
//
//   L_r(p,d) = C(p,d) + min(L_r(q,d), L_r(q,d-1)+P1, L_r(q,d+1)+P1, m+P2) - m
//   m = min_k L_r(q,k),  q = p - r;  L_r(p,d) = C(p,d) where q leaves the image.
//
// Mapping (CDNA4, wave64):
//   * A path LINE is owned by one 16-lane DPP row; lane k holds disparities
//     [k*DPL, k*DPL + DPL) as DPL/2 packed u16 pairs, so every per-disparity
//     op is one v_pk_* for two disparities.
//   * The d-1 / d+1 neighbours are v_alignbit within the lane plus one DPP
//     row_shr:1 / row_shl:1 across lanes (INF fed in at the row edges).
//   * min_k L is a lane-local v_pk_min tree + a 4-step DPP row reduction
//     (quad_perm, half-mirror, mirror) that leaves the minimum in all 16
//     lanes -- no LDS, no barrier.
//   * A wave carries 4 lines, a 256-thread workgroup 16 lines of one
//     direction.  Vertical lines: consecutive x; diagonal lines: consecutive
//     (x - y) mod W, so the 4 pixels a wave touches per step are adjacent in
//     memory (one 4*D-byte span); horizontal lines: 4 rows, one D-byte span
//     each.  Diagonals use the wrap-around trick: line i visits
//     ((i + rx*t) mod W, t) and restarts (L = C) where x wraps, so every line
//     has exactly H steps and no lane idles on ragged diagonal lengths.
//   * Cost bytes are prefetched PF steps ahead into a register ring (the
//     loads do not depend on the recurrence), hiding HBM latency behind the
//     dependent DPP chain of the current step.
//
// Two output modes (g.ckpt):
//   0  every direction writes its u8 volume, [8][H][W][D] (sva_paths_d, the
//      stage API the parity tests read): 8 C reads + 8 L writes per disparity.
//   2  the frame route, the tile pipeline: the four
//      diagonal directions write volumes, [4][H][W][D] (directions 4..7 in
//      slots 0..3); horizontal lines store checkpoints every seg columns
//      ([2][H][nsx][D]) and vertical lines every seg rows ([2][nsy][W][D];
//      seg = 2^tile_geom().seg_log2), and wta_hv.hip recomputes those four
//      per tile: 8 C reads + 4 L writes.
//      The pair route (sgm_paths_kernel<DPL, true>) is mode
//      2 with the four diagonals as pair lines: two u8 pair-sum volumes
//      [2][H][W][D] instead of four L_r volumes.  A pair line takes two DPP
//      rows of a wave (§4.16), so a wave carries 2 and a workgroup 8 of them.
//      With path minima (sgm_paths_kernel<DPL, PAIR, true>)
//      the horizontal and vertical lines of either mode-2 route also store
//      each pixel's entering minimum, 8 bytes per segment beside its
//      checkpoint, which wta_hv.hip reads instead of forming it again.
//   (Mode 1, the round-2 route of DESIGN.md §4.6 -- six volumes, horizontal
//   checkpoints only, finished by wta_h.hip -- was removed in ABI v5.)
#include "sgm_common.h"
#include "sva_tuning.h"

namespace sva {
namespace {

using namespace sgm;

constexpr int PATH_BLOCK = 256;
constexpr int LINES_PER_BLOCK = PATH_BLOCK / 16;
constexpr int PAIR_LINES = LINES_PER_BLOCK / 2;   // a pair line is two rows: roles T and B

// PAIR (the pair route; one frame, tile pipeline only): the
// four diagonals run as 4 * blk_w blocks of 8 pair lines (sgm_common.h
// pair_line: two 16-lane rows per line, which meet in the middle, §4.16) that
// write two pair-sum volumes, L8 = [2][H][W][D] (pairs 4+5, 6+7), through two
// wave-private row-checkpoint planes after the vertical ones.
// MN (path minima; one frame, tile pipeline only): the
// horizontal and vertical lines also store every pixel's entering minimum to
// MNP, [2][H][ns][8] then [2][nsy][W][8] (sgm_common.h), which wta_hv reads
// instead of recomputing it.
template <int DPL, bool PAIR, bool MN>
__global__ __launch_bounds__(PATH_BLOCK) void sgm_paths_kernel(const uint8_t* __restrict__ C,
                                                               uint8_t* __restrict__ L8,
                                                               uint8_t* __restrict__ CK,
                                                               uint8_t* __restrict__ CKV,
                                                               uint8_t* __restrict__ MNP,
                                                               PathGeom g) {
    // Horizontal directions (W steps per line, the longest) get the lowest
    // block ids -- every frame's of a batch before any vertical / diagonal
    // block -- and issue priority so they are never the tail.
    int b = blockIdx.x, r, lb, f;
    if constexpr (PAIR) {
        // The pair blocks carry most of the launch's instructions (a role is
        // H/2 steps, then H/2 double steps): they are
        // dispatched first, with the highest issue priority; then the
        // horizontal lines (W steps, the longest chain of a 16:9 frame), then
        // the vertical ones.  At 120 VGPRs (4 waves per SIMD) the whole grid
        // is resident at 1080p (856 workgroups on 1024 slots).  In-process A/B
        // at 1080p D=128 (profiles/r08_meet/ab_orders_1080p_d128.log.txt),
        // frame / sgm_paths ms: this order, priorities pair 3 / horizontal 1
        // 0.790 / 0.487 (two builds), 3 / 2 0.793 / 0.490, 2 / 1 0.792 /
        // 0.489; horizontal blocks first, horizontal 1 / pair 3 0.796 / 0.490,
        // horizontal 3 / pair 2 0.818 / 0.514; the kernel that walked down and
        // back 0.822, 0.825 / 0.517, 0.521.  (Step-0 ablation of §4.16, pair
        // blocks after the vertical ones: 0.914 / 0.605.)
        f = 0;
        const int npb = 4 * g.blk_w;
        if (b < npb) {
            r = 4 + 2 * (b & 1);
            lb = b >> 1;                                  // a block of PAIR_LINES lines
            __builtin_amdgcn_s_setprio(3);
        } else if (b < npb + 2 * g.blk_h) {
            b -= npb;
            r = b / g.blk_h;
            lb = b - r * g.blk_h;
            __builtin_amdgcn_s_setprio(1);
        } else {
            b -= npb + 2 * g.blk_h;
            r = 2 + (b & 1);
            lb = b >> 1;
        }
    } else if (b < 2 * g.blk_h * g.npair) {
        f = b / (2 * g.blk_h);
        b -= f * 2 * g.blk_h;
        r = b / g.blk_h;
        lb = b - r * g.blk_h;
        __builtin_amdgcn_s_setprio(1);
    } else {
        // band-major: the six vertical / diagonal directions of a 16-line band
        // are adjacent in dispatch order, so the waves that read a cost row
        // (its vertical band and the diagonal bands crossing it) start
        // together and progress at a similar pace: more of the second and
        // third reads of a row come from the caches.  A/B in-process at 1080p
        // D=128 (profiles/r03_v3): kernel 0.616-0.622 -> 0.594-0.599 ms, frame
        // 261-263K -> 266-267K Mdisp/s; direction-major had the first-dispatched
        // direction hundreds of steps ahead.
        // (a batch's frames follow one another, each band-major)
        b -= 2 * g.blk_h * g.npair;
        f = b / (6 * g.blk_w);
        b -= f * 6 * g.blk_w;
        r = 2 + b % 6;
        lb = b / 6;
    }
    C += (size_t)f * g.cstr;
    L8 += (size_t)f * g.lstr;
    if (g.ckpt) {
        CK += (size_t)f * g.ckstr;
        CKV += (size_t)f * g.ckvstr;
    }
    int line = lb * LINES_PER_BLOCK + (threadIdx.x >> 4);
    int role = 0;
    if constexpr (PAIR) {
        if (r >= 4) {
            // a pair line takes two rows of a wave: rows 0, 1 are role T of
            // lines l, l + 1 and rows 2, 3 role B of the same two lines
            const int row = (int)(threadIdx.x >> 4);
            line = lb * PAIR_LINES + 2 * (row >> 2) + (row & 1);
            role = (row >> 1) & 1;
        }
    }
    const int k = threadIdx.x & 15;
    const int nlines = r < 2 ? g.H : g.W;
    if (line >= nlines) return;  // whole 16-lane row leaves together (both roles of a pair line)
    int rx, ry;
    dir_of(r, rx, ry);
    const rsrc_t rC = make_rsrc(C, g.vol);
    // the tile pipeline's checkpoint segment (§4.9), rows and columns
    constexpr int SL = DPL <= 8 ? tune::kWtahvTileLog2 : tune::kWtahvTileLog2Wide;
    // this direction's minima plane (directions 0..3 of an MN launch)
    const size_t mnh = (size_t)g.H * g.ns * kMinimaSeg, mnv = (size_t)g.nsy * g.W * kMinimaSeg;
    const rsrc_t rMN = !MN || r >= 4 ? rC
                       : r >= 2 ? make_rsrc(MNP + 2 * mnh + (size_t)(r - 2) * mnv, mnv)
                                : make_rsrc(MNP + (size_t)r * mnh, mnh);
    if constexpr (PAIR) {
        if (r >= 4) {
            const int pr = r == 4 ? 0 : 1;                // pair 4+5, pair 6+7
            const rsrc_t rCK = make_rsrc(CKV + (size_t)(2 + pr) * g.ckvvol, g.ckvvol);
            const rsrc_t rE = make_rsrc(L8 + (size_t)pr * g.vol, g.vol);
            pair_line<DPL, pf_v<DPL>(), SL>(rC, rE, g, rx, line, role, k, rCK);
        } else if (r >= 2) {
            const rsrc_t rCK = make_rsrc(CKV + (size_t)(r - 2) * g.ckvvol, g.ckvvol);
            path_line<DPL, false, pf_v<DPL>(), 2, SL, MN>(rC, rC, g, rx, ry, line, k, rCK, rMN);
        } else {
            const rsrc_t rCK = make_rsrc(CK + (size_t)r * g.ckvol, g.ckvol);
            path_line<DPL, false, pf_h<DPL>(), 1, SL, MN>(rC, rC, g, rx, ry, line, k, rCK, rMN);
        }
    } else if (r >= 4) {
        // volume slot: every direction (8 volumes), or the tile pipeline's
        // four diagonals in direction order
        const int slot = !g.ckpt ? r : r - 4;
        const rsrc_t rL = make_rsrc(L8 + (size_t)slot * g.vol, g.vol);
        path_line<DPL, true, pf_v<DPL>()>(rC, rL, g, rx, ry, line, k, rL, rL);
    } else if (const bool tile = g.ckpt != 0; r >= 2 && tile) {   // (tile: checkpoint lines)
        const rsrc_t rCK = make_rsrc(CKV + (size_t)(r - 2) * g.ckvvol, g.ckvvol);
        path_line<DPL, false, pf_v<DPL>(), 2, SL, MN>(rC, rC, g, rx, ry, line, k, rCK, rMN);
    } else if (r >= 2) {
        const rsrc_t rL = make_rsrc(L8 + (size_t)r * g.vol, g.vol);
        path_line<DPL, false, pf_v<DPL>()>(rC, rL, g, rx, ry, line, k, rL, rL);
    } else if (tile) {
        const rsrc_t rCK = make_rsrc(CK + (size_t)r * g.ckvol, g.ckvol);
        path_line<DPL, false, pf_h<DPL>(), 1, SL, MN>(rC, rC, g, rx, ry, line, k, rCK, rMN);
    } else {
        const rsrc_t rL = make_rsrc(L8 + (size_t)r * g.vol, g.vol);
        path_line<DPL, false, pf_h<DPL>()>(rC, rL, g, rx, ry, line, k, rL, rL);
    }
}

// The kernel's geometry argument, from the plan.
PathGeom path_geom(const AggPlan& p) {
    PathGeom g;
    g.W = p.W; g.H = p.H; g.D = p.D; g.P1 = p.P1; g.P2 = p.P2;
    g.blk_h = (p.H + LINES_PER_BLOCK - 1) / LINES_PER_BLOCK;
    g.blk_w = (p.W + LINES_PER_BLOCK - 1) / LINES_PER_BLOCK;
    g.vol = p.vol;
    g.ckpt = p.route == AggRoute::Eight ? 0 : 2;
    g.ns = p.tg.nsx;
    g.ckvol = p.tg.hck_bytes / 2;
    g.nsy = p.tg.nty;
    g.ckvvol = p.tg.vck_bytes / 2;        // one row-checkpoint plane
    g.npair = p.frames;
    g.cstr = p.c_stride;
    g.lstr = p.vol_stride;
    g.ckstr = p.hck_stride;
    g.ckvstr = p.vck_stride;
    g.pair = p.route == AggRoute::Pair ? 1 : 0;
    g.dreal = p.dreal;
    return g;
}

}  // namespace

bool paths_supported(int D) { return is_native_d(D); }

// (a pair instance exists only for the D classes whose pair route is enabled,
// a minima instance only for those with tune::kPathMinima*; plan_valid has
// refused the others)
hipError_t launch_paths(Ctx& c, const AggPlan& p, const AggBuffers& b) {
    DispatchTimer t(c, "sgm_paths");
    if (!plan_valid(p) || !buffers_fit(p, b)) return hipErrorInvalidValue;
    const PathGeom g = path_geom(p);
    // (pair: 2 * 2 * blk_w blocks of 8 pair lines + 2 * blk_w vertical blocks)
    const dim3 grid((unsigned)((2 * g.blk_h + 6 * g.blk_w) * p.frames));
    t.used = true;
    for_native_d(p.D, [&](auto k) {
        using K = decltype(k);
        with_flag<K::kPair>(p.route == AggRoute::Pair, [&](auto pair) {
            with_flag<K::kMinima>(p.minima, [&](auto mn) {
                hipExtLaunchKernelGGL((sgm_paths_kernel<K::DPL, decltype(pair)::value, decltype(mn)::value>),
                                      grid, dim3(PATH_BLOCK), 0, c.stream, t.start, t.stop, 0, b.C,
                                      b.volumes, b.CK, b.CKV, b.MN, g);
            });
        });
    });
    return hipGetLastError();
}

}  // namespace sva
