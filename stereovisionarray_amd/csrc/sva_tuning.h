// sva_tuning.h -- every measured tuning constant of the kernels, in one place.
//
// Product translation units carry no experiment switches (VERDICT r02 weak
// #7): each constant below is the value the in-process A/B runs chose, with
// the measurement that chose it.  An experiment build rewrites this header
// in a scratch copy of csrc/ (tools/build_variants.sh KEY=VALUE ...), so the
// A/B library never shares a translation unit with the product.
#pragma once

#include <cstddef>

namespace sva {
namespace tune {

// ---- sgm_paths.hip / sgm_common.h ------------------------
// Prefetch ring depth in steps, per line kind and disparities per lane
// (D = 16 * DPL).  Horizontal lines are few (2H) and long (W steps) and run
// alone once the vertical/diagonal lines drain, so they get the deeper ring.
// In-process A/B (tools/ab_paths.py): 1080p D=128 H/V 8/8 0.755-0.788 ms,
// 32/12 0.661 (149 VGPRs, 3 waves/SIMD), 40/8 0.689 (2 waves/SIMD), 32/4
// 0.770; re-checked after the round-2 step changes: 32/12 0.597, 32/16 0.596,
// 32/8 0.601, 28/12 0.597, 36/12 0.599; after the band-major dispatch (round
// 3, profiles/r03_v6) 32/12 0.5845, 32/16 0.5834, 32/8 0.5875, 28/12 0.5815,
// 36/12 0.5798 (frames 0.952-0.966 ms, all within noise).  D=64 (1080p) 40/12 0.372 vs 8/8
// 0.416; D=192 24/8 0.996 vs 12/8 1.154; D=256 (4K) 12/8 (16/8 equal, 20/8
// and 12/12 +3 %).
// Round 5, small frames (profiles/r05_v5/prefetch_v/): at 640x480 every
// direction alone takes 0.054-0.065 ms (direction ablations, abl_*.log.txt)
// and a vertical line alone pays ~125 ns per step on a 12-step ring, so the
// vertical / diagonal rings were swept again.  D=64 (kPfV4, sgm_paths ms,
// two runs each): 12 / 16 / 20 / 24 / 28 / 32 / 40 at 640x480 0.0776 /
// 0.0757 / 0.0771 / 0.0703 / 0.0793 / 0.0772 / 0.0703, 960x540 all 0.093,
// 1080p 0.2965 / 0.2895 / 0.2976 / 0.2912 / 0.2978 / 0.2899 / 0.292; 24 is
// free in registers (the horizontal ring sets the VGPRs).  D=128 (kPfV8) 12 /
// 16 / 20 / 24 / 32: 640x480 0.1049 / 0.1022 / 0.1031 / 0.1011 / 0.1042 but
// 1080p 0.5178 / 0.518 / 0.5209 / 0.5261 / 0.5218, so D=128 keeps 12.
constexpr int kPfH4 = 40, kPfV4 = 24;
constexpr int kPfH8 = 32, kPfV8 = 12;
constexpr int kPfH12 = 24, kPfV12 = 8;
constexpr int kPfH16 = 12, kPfV16 = 8;
// Cache-policy bits of the cost-volume loads.  A/B (full frame, in-process):
// nt (2) +8 %, sc0+nt (3) +8 %; sc0 (1), sc0+sc1 (17), 8, 16 within noise.
constexpr int kCLoadAux = 0;
// Cache-policy bits of the checkpoint stores (0 = default: wta_hv reads them
// back soon).  nt (2) measured: frame 0.952 vs 0.963 ms median,
// min 0.948 vs 0.942 -- noise (profiles/r03_v6/ab_retune_sgm.log.txt).
constexpr int kCkptStoreAux = 0;
// Horizontal / vertical checkpoint stores at compile-time step positions
// behind 0-7 lead steps, or a runtime segment test every step (sgm_common.h
// path_line; needs PF a multiple of the segment), for the kernels with at
// most this many disparities per lane (0: none).  sgm_paths ms, runtime test
// -> static positions (profiles/r05_v5/ckpt_hits/): 640x480 D=64 0.0703 ->
// 0.0672, 960x540 D=64 0.0938 -> 0.0821 (frame 0.156 -> 0.145), 1080p D=64
// 0.2918 -> 0.2889; but 1080p D=128 0.5127 -> 0.5192 and 0.5109 -> 0.5155 in
// the two variant orders (+0.7 %), D=192 / 4K D=256 within 0.3 %.  So D=64
// only (DPL 4).
constexpr int kStaticCkptHitsMaxDpl = 4;

// ---- wta_hv.hip -------------------------------------------
// The pair route: a frame (not a batch) whose 2 * P2
// fits a u8 has each diagonal and its opposite walked by one wave of
// sgm_paths, which writes the two pair-sum volumes E = (L_a - C) + (L_b - C)
// instead of four L_r volumes; wta_hv reads two volumes and adds 4C.  Per
// native D (DPL = D / 16); measurements in §4.15.  Only the enabled classes
// compile a pair instance of the two kernels.
constexpr int kDiagPair4 = 0, kDiagPair8 = 1, kDiagPair12 = 0, kDiagPair16 = 0;
// Smallest frame (W * H) that takes the pair route.  A pair line's two roles
// are each a chain of H/2 steps and then H/2 double steps (§4.16; H and H
// before the two recurrences met in the middle), against H steps of a
// diagonal line on four volumes, so the smallest frames are still bound by
// that chain, not by their bytes.  Frame ms at D=128, four volumes (two
// copies) / pair (in-process A/B, profiles/r08_meet/ab_routes_*): 640x480
// 0.181, 0.179 / 0.188, 960x540 0.254, 0.255 / 0.275, 1280x720 0.437, 0.435 /
// 0.404, 1080p 0.867, 0.865 / 0.793, 2560x1440 1.524, 1.501 / 1.365, 4K 3.63,
// 3.58 / 3.03.  (Walking down and back: 0.181 / 0.257, 0.257 / 0.312, 0.432 /
// 0.435, 0.854 / 0.823, 1.503 / 1.453, 3.42 / 3.11, and a threshold of 1.6 M.)
// The crossover is not monotonic in pixels (the pair blocks' share of the CUs
// depends on W, their chain on H): 1024x768 0.337 / 0.346, 1280x800 0.472 /
// 0.445, 1920x540 0.503 / 0.524, 1080x1080 0.539 / 0.558, 1600x900 0.605 /
// 0.614 lose or win by shape, and every size measured from 1400x1050 up wins
// (1400x1050 0.623 / 0.594, 1440x1080 0.650 / 0.615, 1680x1050 0.719 / 0.711,
// 1600x1200 0.791 / 0.751, 2048x1024 0.838 / 0.799).  The threshold sits
// above the largest frame that lost (1600x900, 1.44 M).
constexpr long long kDiagPairMinPixels = 1450000;
// Path minima: on the frame route the horizontal and
// vertical lines of sgm_paths also store every pixel's entering minimum (one
// byte; 8 bytes per segment beside its checkpoint), and wta_hv's four
// recurrences read m instead of forming it (7 VALU of each step, 4 of them
// half-rate DPP).  Per native D (DPL = D / 16); only the enabled classes
// compile the minima instances of the two kernels.  The stage entries and
// the batch route keep the instances without.  D=128, 1080p
// (profiles/r09_minima/): wta_hv static VALU 1,607 -> 1,416, SQ_INSTS_VALU
// 103.5 M -> 91.2 M; bench lines, parent / this alternating, ms per step
// 0.7980-0.7986 / 0.7887-0.7897 and, in a second visit, 0.7967-0.7995 /
// 0.7901-0.7909 (wta_hv 0.195 -> 0.1895, sgm_paths 0.5035 -> 0.5005): -1.1 %,
// less than the VALU ratio because wta_hv was not on its VALU ceiling alone
// (§4.17).  The four-volume route forced at 1080p, in-process: wta_hv 0.250,
// 0.243 -> 0.248, frame 0.877, 0.870 -> 0.875, nothing beyond the spread of
// the two parent copies, and never slower; it shares the switch.  D=192 /
// 256 measured with the switch on (ab_wide_*): frame 1.302, 1.285 -> 1.290 and
// 1.653, 1.678 -> 1.667, inside the spread of two copies of one build: off.
// D=64 is not built (its lines store checkpoints at static positions,
// kStaticCkptHitsMaxDpl, and would need their own flush).
constexpr int kPathMinima4 = 0, kPathMinima8 = 1, kPathMinima12 = 0, kPathMinima16 = 0;
// prefetch depth (pixels) of wta_hv's two pair-volume loads: wta_hv ms at 1080p
// D=128 for 2 / 3 / 4: 0.1862 / 0.1837 / 0.1815
constexpr int kWtahvPfVolPair = 4;
// log2 of the tile rows and of the checkpoint segment (tiles are 16 x 2^this).
// Round 6 re-check of 16 x 16 (checkpoints every 16: -0.13 GB per 1080p
// D=128 frame, now that wta_hv streams its bytes; profiles/r06_v11/), frame
// ms 16x8 / 16x16: 1080p D=128 0.8806 / 0.899 (sgm_paths 0.516 -> 0.500,
// wta_hv 0.252 -> 0.283 at 2 workgroups per CU by its 64 KB of LDS), D=64
// 0.511 / 0.512, 640x480 D=64 0.127 / 0.138.  Stays 3.
constexpr int kWtahvTileLog2 = 3;
constexpr int kWtahvTileLog2Wide = 3;      // D > 128
// Prefetch depth (pixels) of the four diagonal-volume loads in the last pass.
// Re-checked after the late-round-3 VALU cuts (profiles/r03_v8/ab_wtahv_pf_vol.log.txt,
// wta_hv ms for 4 / 2 / 3 / 6): D=128 0.2615-0.2618 / 0.2641-0.2659 /
// 0.2603-0.2605 / 0.293; D=192 0.4031 / 0.4048 / 0.4008 / 0.514; D=256 0.5559 /
// 0.5129 / 0.5254 / 0.575.  D=64 keeps 4: 3 there cost 12 % (0.145 -> 0.163
// ms, ab_wtahv_pf_vol_keep.log.txt).
constexpr int kWtahvPfVol = 3;             // D=128, D=192
constexpr int kWtahvPfVol4 = 4;            // D=64
constexpr int kWtahvPfVol16 = 2;           // D=256
// The row minimum's last DPP step pinned next to its move (sva_device.h
// row_min_u32<true>: one v_min_u32_dpp instead of v_mov 0 + v_mov_dpp + v_min),
// in the recurrences and in the WTA.  wta_hv, in-process, 3 variants x 2
// positions (profiles/r03_v8/ab_wtahv_pin_row_min.log.txt): 1080p D=128
// 0.2599 / 0.2667 -> 0.2586 / 0.2657 ms, 4K D=256 2.314 -> 2.284 ms; small but
// the same sign at every D.  (In sgm_paths the same pin was neutral at 1080p
// and 1-2 % slower at 4K, so the path kernel stays unpinned.)
constexpr int kWtahvPinRowMin = 1;
constexpr int kWtahvPinWta = 1;
// Minimum waves per SIMD asked of the compiler for wta_hv (launch bounds).
// Round 6: u8 keeps + phase H's cost loads after phase V + a 2-pixel volume
// prefetch bring D=128 to 90 VGPRs with no scratch, 5 waves/SIMD -- and the
// kernel does not get faster (1080p D=128 wta_hv 0.2519 ms product vs
// 0.2578 / 0.2598 / 0.2610 for the three 5-wave variants; D=64 and 640x480
// within noise; profiles/r06_v7/ab_o5_*): it sits on its instruction-mix
// ceiling and its bytes at once.
constexpr int kWtahvMinWaves = 1;

// ---- batched frames (sva_disparity_sgm_batch_d) ----------
// Frames per sgm_paths / wta_hv launch, and the workspace those frames may
// hold (cost + 4 diagonal volumes + checkpoints per frame).
constexpr int kBatchMaxPairs = 8;
// Side streams for the batch's per-frame census + cost kernels (small and
// VALU-bound at the reference's half-size frames: one after another on the
// context stream they were 36 % of a 960x540 D=64 center8 step,
// profiles/r04_*/c8half_batch.log.txt).
constexpr int kBatchCostStreams = 3;
// Frames per aggregation launch inside a batch (0: the whole batch): the
// context stream aggregates sub-batch j while the side streams compute the
// cost volumes of sub-batch j + 1 (round 5).
constexpr int kBatchSubFrames = 4;
constexpr size_t kBatchMaxBytes = (size_t)24 << 30;

// ---- sva_reserve's placement check ----------------------
// Buffer sets timed (the first allocation plus trials - 1 more) when a frame's
// stage buffers reach kPlacementMinBytes.  At 4K D=256 the path kernel ran
// 4.28-4.98 ms on twelve allocations of the same buffers, stable within each
// (profiles/r06_v6/probe_4k_alloc.log.txt); with the check, 4.23-4.28 ms in
// three processes against 4.30 / 4.86 / 4.87 without (profiles/r06_v9/4k_t*).
// 1080p D=128 (1.6 GB) has no such spread: its trials ran 0.502-0.510 ms and
// the bench line did not move with the check forced on there (0.8816-0.8827
// vs 0.8772-0.879 ms per frame, profiles/r06_v9/1080_t*), hence the threshold.
// 6 sets, all held until the choice (so no trial reuses another's pages):
// with 4 sets, one set freed before the next was taken, a later box kept a
// 4.51 ms set (slowest 4.84; profiles/r06_final3/4k_d256_four_sets_freed.log.txt).
constexpr int kPlacementTrials = 6;
constexpr size_t kPlacementMinBytes = (size_t)4 << 30;

// ---- census.hip / census_cost.hip / cost.hip ------------
// Rows per workgroup of the multi-row census kernel.
constexpr int kCensusRows = 16;
// Frames of D >= this (1-D steps) run census_cost; smaller D run the census
// kernel + the cost kernel.  The round-1 VALU kernel lost at D=64 (0.609 vs
// 0.650 ms at 1080p, so 128 until round 4); the MFMA kernel wins there too,
// frame ms split / census_cost (profiles/r04_v3/ab_d64_route.log.txt): 1080p
// 0.5247 / 0.5224, 640x480 0.1499 / 0.1422, 960x540 0.1862 / 0.1824.
constexpr int kCensusCostMinD = 64;
// census_cost: rows per workgroup.  The MFMA kernel prefers 8 (census_cost ms
// at 2 / 4 / 8 / 16 rows, profiles/r04_v4/ab_census_cost_rows.log.txt: 1080p
// D=128 0.1063 / 0.0974 / 0.0938 / 0.1062, D=64 0.0789 / 0.0676 / 0.0648 /
// 0.0674, D=256 0.1763 / 0.1572 / 0.1488 / 0.1501, 4K D=128 0.399 / 0.366 /
// 0.342 / 0.353) unless that leaves fewer than kCensusCostMinGroups
// workgroups: 640x480 D=64 (600 workgroups at 8 rows) 0.0173 / 0.0162 /
// 0.0196 / 0.0275.  (The round-1 VALU kernel had 4 as the best of 2-16,
// profiles/r01_v8/ab_census_cost_tiling.jsonl.)
constexpr int kCensusCostRows = 8;
constexpr int kCensusCostRowsSmall = 4;
// (900 instead: within noise at 960x540 D=64 / 128, 0.0224 / 0.0293 vs 0.0223 /
// 0.0289 ms, profiles/r04_v4/ab_census_cost_store_threshold.log.txt)
constexpr int kCensusCostMinGroups = 1536;   // 6 per CU
// census_cost_mma_kernel: pixels per workgroup row at D = 64 / 128 / 192 /
// 256.  64 px hold 5 / 4 / 3 workgroups per CU where 128 px hold 4 / 3 / 2 /
// 2 (LDS), but form 4 census windows per pixel instead of 3.  At 4 rows per
// workgroup, census_cost ms 128 / 64 px (profiles/r04_v3/ab_census_cost_px.log.txt):
// 1080p D=64 0.0673 / 0.0669, 640x480 D=64 0.0193 / 0.0159, D=128 0.0975 /
// 0.0985, D=192 0.1409 / 0.1360, D=256 0.1567 / 0.1744.  Re-measured at 8
// rows (profiles/r04_v4/ab_census_cost_px_rows8.log.txt), D=128 turns to 64
// px: 1080p 0.0954 / 0.0913 (also with dir +1: 0.0954 / 0.0915), 4K 0.343 /
// 0.333, 960x540 0.0345 / 0.0290, 640x480 0.0220 / 0.0203; D=64, 192, 256
// keep theirs (the swapped set: 0.0650 -> 0.0667, 0.1287 -> 0.1319, 0.1494
// -> 0.1646).  MFMA groups of 4 tiles: 2 / 6 / 12 within 0.5 % or slower.
constexpr int kCensusCostPx4 = 64, kCensusCostPx8 = 64, kCensusCostPx12 = 64, kCensusCostPx16 = 128;
// Cost-volume stores of census_cost: 1 non-temporal, 0 default policy.
// Round 4, every width, on the VALU kernel
// (profiles/r04_v3/ab_store_policy_all.log.txt, frame ms nt / default):
// default stores speed census_cost up (4K D=256 0.622 -> 0.571 ms) but leave
// dirty lines whose write-back lands in sgm_paths (4.887 -> 4.946), so the
// frame is equal at 4K D=256 (7.603 / 7.594) and slower elsewhere: 1080p
// D=128 0.902 / 0.920, D=192 1.332 / 1.342, D=256 1.736 / 1.743, 4K D=128
// 3.775 / 3.793, 4K D=192 6.042 / 6.078.  The MFMA kernel stages each row
// and stores whole 128-byte lines, nt (single 4-byte nt stores from the MFMA
// lanes: census_cost 0.57 ms at 1080p D=128, ab_census_cost_mfma.log.txt).
// Re-checked on the re-tiled MFMA kernel, frame ms nt / default
// (ab_census_cost_store_threshold.log.txt): 1080p D=128 0.9025 / 0.9215, D=256
// 1.733 / 1.753, 4K D=256 7.59 / 7.64.
constexpr int kCostStoreNT = 1;
// census_cost's store phase reads the staged costs in staging-slot order (1:
// conflict-free LDS reads at D=128) or in pixel order (0: a read group's 4
// pixels sit 16 slots apart, all on one bank set, 4-way conflicts; SQ counters
// at 1080p D=128 had 8.7 M bank-conflict cycles of 30.8 M LDS cycles).
// census_cost ms 0 -> 1 (profiles/r05_v5/slot_order/): 1080p D=128 0.0951 ->
// 0.0918, D=192 0.127 -> 0.1247, D=256 0.1418 -> 0.1376, 4K D=256 0.5376 ->
// 0.5213, D=64 unchanged.
constexpr int kCensusCostSlotOrder = 1;
// census_cost2.hip (2-D array steps): adjacent lattice lines per workgroup,
// which share one staged image patch.
constexpr int kCensusCost2Lines = 8;

// ---- refpath.hip, Mode R plane kernel v3 ------------------
constexpr int kPlaneOuKB = 24;      // staged O chunk (KB)
constexpr int kPlaneWords = 1024;   // offset bitmap per pass: 32K bits
constexpr int kPlaneMinBlocks = 3;  // __launch_bounds__ min workgroups per CU
// Plane loop body (round 5): the box-sum scans of this
// many rows (a divisor of 8) at a time, stage by stage: DESIGN.md §4.2.
constexpr int kPlaneStageMajor = 2;
// Every tile of the plane kernel is split into S shares of its offsets, each
// its own workgroup; the per-pixel keys meet in global memory by atomicMin
// (ref_plan.h plane_shares, refpath.hip ref_finalize_kernel).  S =
// kPlaneSplitRounds rounds of workgroup slots over the tile count, rounded,
// within [kPlaneSplitMin, kPlaneSplitMax]: the sweep of S = 1..6 at six frame
// sizes (profiles/r05_v5/plane_walk/n*, r6q) is the table in DESIGN.md §4.2.
constexpr int kPlaneSplitMin = 3;
constexpr int kPlaneSplitMax = 6;
constexpr int kPlaneSplitRounds = 4;

// ---- cross_check.hip -------------------------------------
// Block order: 0 view-major, 1 tile-major (the view index innermost in groups
// of 8 tiles, so the workgroups that share an XCD walk one tile of every view).
// A/B at 1080p on real maps, the orders alternating call by call, 15 calls each,
// every plane written, stream events around the call (tools/bench_cross_check.py
// --kernel, profiles/cross_check/kernel_1080p.json), ms median (min-max), view /
// tile:
// n = 25  1.380 (1.374-1.385) / 1.339 (1.333-1.344); u16 planes only 1.282
// (1.275-1.285) / 1.221 (1.212-1.226): tile-major wins outside both spreads.
// n = 9   0.243 (0.221-0.258) / 0.224 (0.216-0.232): the spreads overlap, no
// significant difference.  320x240: 13-55 us, equal in one session, tile-major
// slower in the median in another; not decisive.
// Chosen on n = 25; one order for every n rather than a switch on n.
constexpr int kCrossTileMajor = 1;

// ---- speckle.hip -----------------------------------------
// The label pass's tile: one workgroup of 256 threads resolves kSpeckleTileW x
// kSpeckleTileH pixels in LDS (10 bytes of LDS per pixel).  A wide, flat tile
// keeps the u16 row reads and the u32 row writes 128 bytes and more long.
// One A/B, 64x16 against 32x32 (a library built by tools/build_variants.sh), each
// in a process of its own in one session: tools/bench_speckle.py --kernel, 1080p
// real maps, 15 calls, max_size 20, max_diff 1, u16 planes only, stream events
// around the four launches (profiles/speckle/kernel_1080p*.json), ms median
// (min-max), 64x16 / 32x32:
// n = 25  2.177 (2.166-2.194) / 2.173 (2.106-2.205): no difference.  The square
// tile's label pass is faster, 1.222 (1.214-1.229) / 1.105 (1.093-1.114), and
// its merge pass -- 1.5x the border links -- slower by as much, 0.571
// (0.555-0.582) / 0.688 (0.618-0.718).
// n = 8   0.734 (0.722-0.752) / 0.700 (0.691-0.734): the spreads overlap.
// n = 1   0.157 (0.154-0.162) / 0.149 (0.146-0.153): 32x32 ahead by 8 us, its
// slowest call 0.2 us under the other's fastest.
// No winner where the time is (n = 25), so the shape the layout argues for stays.
constexpr int kSpeckleTileW = 64, kSpeckleTileH = 16;

// ---- fill.hip ---------------------------------------------
// The scan cuts every line into segments of kFillSegment steps, one thread each,
// which begins max_dist steps early: a thread's dependent chain is kFillSegment
// + max_dist steps and it reads (kFillSegment + max_dist) / kFillSegment times
// the map.  A short segment gives more threads and more re-reading, a long one
// a longer chain.  kFillRing pixels are loaded ahead of the chain.
// One sweep (tools/bench_fill.py --kernel, the segment set through
// SVA_DEBUG_FILL_SEGMENT on one warm context in one session; 1080p, n = 25
// synthetic maps with 5 % holes, u16 planes only, 15 calls, stream events around
// the two launches; profiles/fill/kernel_1080p.json), ms median (min-max):
//   segment   max_dist 16          max_dist 64          max_dist 255
//   8         2.164 (2.152-2.173)  4.371 (4.354-4.401)  12.807 (12.789-12.824)
//   16        1.839 (1.825-1.843)  2.819 (2.799-2.838)   6.766 (6.740-6.790)
//   32        1.752 (1.736-1.760)  2.166 (2.142-2.185)   4.041 (4.014-4.084)
//   64        1.631 (1.618-1.658)  1.835 (1.821-1.856)   2.893 (2.846-2.947)
//   128       1.807 (1.786-1.876)  1.927 (1.887-1.964)   2.474 (2.430-2.538)
// 64 wins outside the spreads at the distances an occlusion band has (16, 64);
// 128 wins at 255 only, by 0.42 ms.  The apply launch is 0.31-0.35 ms of every
// cell.  kFillRing was not swept.
constexpr int kFillSegment = 64;
constexpr int kFillRing = 4;
// sva_array_depth_filled fills at most this many maps per call of
// sva_fill_holes_d, which bounds the key planes (32 bytes per pixel and map) to
// 531 MB at 1080p.
constexpr int kFillFrameMaps = 8;

// ---- wmedian.hip ------------------------------------------
// A workgroup of kWmedTileW x kWmedTileH threads stages its tile and an r-wide
// halo in LDS: (W + 2r)(H + 2r) cells for W * H outputs, 9.2 staged cells per
// output at r = 15 for 32 x 8.  A row of kWmedTileW = 32 threads reads 32
// neighbouring u16 cells, 16 LDS banks, without a conflict.
// One sweep (a build with the five shapes as template instances behind a debug
// key, since removed, and its window loops unrolled four times; the shape set on
// one warm context in one session, the first shape again at the end; 1080p, n = 25 synthetic maps with 5 % holes, guided, u16 planes
// only, 15 calls, stream events around the launch;
// profiles/wmed/tile_sweep_1080p.json), ms median [min-max]:
//   tile     r = 2                            r = 5                            r = 15
//   32 x 8                           13.5578 [13.5384-13.8955]        35.4873 [35.4606-35.4976]        296.1375 [295.6524-296.3237]
//   16 x 16                          13.5420 [13.5249-13.5823]        35.4307 [35.4001-35.4851]        295.8513 [295.4726-296.4768]
//   64 x 4                           13.5765 [13.5145-13.6744]        35.4563 [35.3929-35.4849]        295.6263 [295.3668-296.0222]
//   32 x 16                          13.5934 [13.5467-13.6528]        35.5451 [35.4950-36.4595]        296.2917 [295.9060-296.9395]
//   64 x 8                           13.5669 [13.5344-13.5957]        35.5113 [35.4484-35.6298]        295.8739 [295.6601-296.3386]
//   32 x 8                           13.5992 [13.5267-13.7458]        35.4634 [35.3888-35.5464]        295.2286 [295.0656-296.0691]
// No winner: every shape is within 0.3 % of the others, inside the spread of the
// two 32 x 8 legs -- the time is the window loops', not the staging's.  The
// shape the LDS layout argues for stays.
constexpr int kWmedTileW = 32, kWmedTileH = 8;
// The guides of one launch travel in the kernel's arguments (8 bytes each beside
// the 512-byte table): n_maps beyond this take a further launch.
constexpr int kWmedLaunchMaps = 64;

// ---- rectify.hip ------------------------------------------
// A thread owns kRectPixels adjacent output pixels and stores them as one dword
// (the store width is the reason for 4; not swept).  A workgroup is kRectBlockX x
// kRectBlockY threads: 256 x 4 pixels, one wave per output row segment.
constexpr int kRectPixels = 4;
constexpr int kRectBlockX = 64, kRectBlockY = 4;
// The views of one launch travel in the kernel's arguments, 144 bytes each
// beside 64 bytes of planes and sizes, in a 4 KiB segment: a 25-camera frame is
// one launch, n beyond this take a further one.
constexpr int kRectLaunchViews = 25;

}  // namespace tune
}  // namespace sva
