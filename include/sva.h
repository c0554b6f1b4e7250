/*
 * sva.h -- C-ABI of libsva.so, the MI355X-native stereo disparity engine.
 *
 * This is the drop-in boundary for the reference's array-stereo cost-volume
 * path.  The reference (Nahuel-M/StereoVisionArray) has no plugin API: its hot
 * loop is written inline in main() (src/CameraStereoVision.cpp:44-95) and
 * reaches helpers through include/functions.h and include/Camera.h.  Each
 * entry point below names the reference code it replaces.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - Every function returns an int status: SVA_OK (0) or an SVA_ERR_* code.
 *     No exception crosses the ABI.  sva_last_error() gives the message of the
 *     last failing call on that context.
 *   - Functions without suffix take HOST buffers and are synchronous.
 *     Functions with suffix _d take DEVICE buffers (hipMalloc'd on the
 *     context's device) and are asynchronous on the context's stream; call
 *     sva_synchronize() (or synchronise the stream yourself) before reading.
 *   - Images are 8-bit grayscale, row-major, row pitch in bytes (>= width).
 *     Every other array is dense (pitch = width).
 *   - An image's base address and its pitch need no alignment (a sub-rectangle
 *     of a larger image, base = parent + y0 * P + x0 with pitch = P, is a valid
 *     image, on the host and on the device), and a plane of `height` rows must
 *     be readable -- an output plane that carries a pitch: writable -- for
 *     height * pitch bytes from its base: the bytes between the rows may be
 *     read, never change a result and keep their values.  (Who needs the whole
 *     extent: the refinement's box kernel, whose loads range over height *
 *     pitch bytes, and the host forms sva_shift_perspective,
 *     sva_improve_with_disparity and sva_resize_half, which upload their input
 *     planes whole; the first two also upload the output plane and copy it
 *     back whole, so its bytes between the rows are rewritten with their own
 *     values, while sva_resize_half copies back the pixels only.  Every other
 *     entry, host or device, touches only the width bytes of each row.)  A
 *     crop that reaches its parent's last row therefore needs x0 more bytes
 *     after it for those calls.  Mode R and the refinement load
 *     aligned 4-byte words, so up to 3 bytes before the base or after that
 *     extent may be read together with a byte inside it; such a word never
 *     crosses a page, which asks nothing of the caller.  (tests/
 *     test_image_views_gpu.py runs every entry at every base and pitch residue
 *     modulo 4.)
 *   - A context owns one device and one stream and is not re-entrant; calls on
 *     different contexts may run concurrently from different host threads.
 *   - There is no CPU fallback: if no HIP device is usable every compute call
 *     fails with SVA_ERR_NO_DEVICE.
 */
#ifndef SVA_H
#define SVA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVA_ABI_VERSION 6

enum {
    SVA_OK = 0,
    SVA_ERR_INVALID_ARG = 1,   /* bad size / pointer / parameter            */
    SVA_ERR_UNSUPPORTED = 2,   /* parameter combination not built           */
    SVA_ERR_DEVICE = 3,        /* HIP runtime error                         */
    SVA_ERR_OUT_OF_MEMORY = 4, /* workspace allocation failed               */
    SVA_ERR_NO_DEVICE = 5      /* no usable HIP device                      */
};

/* Mirrors class Camera (include/Camera.h:6-21): public f, pos3D, pixel_size. */
typedef struct sva_camera {
    double f;
    double pos[3];
    double pixel_size;
} sva_camera;

/* Mode S parameters.  Use sva_sgm_params_default(). */
typedef struct sva_sgm_params {
    int32_t D;           /* disparity count, 1..256 (whole-frame entry points; the
                            stage entry points take 64, 128, 192 or 256).  Other
                            D run at the next of those widths with the extra
                            disparities masked out              */
    int32_t dmin;        /* first disparity                                        */
    int32_t dir;         /* x component of the match step: +1: x+(dmin+d) in the
                            other image, -1: x-(dmin+d) (rectified horizontal);
                            see dir_y for array baselines                          */
    int32_t P1;          /* small-jump penalty (default 10)                        */
    int32_t P2;          /* large-jump penalty (default 120); 0 <= P1, P2 <= 193    */
    int32_t subpixel;    /* 1: also write the f32 parabola sub-pixel map          */
    int32_t lr_check;    /* 1: left/right consistency check       */
    int32_t lr_max_diff; /* max |dL - dR| kept by the check (default 1)            */
    uint16_t invalid;    /* disparity written for pixels the check rejects         */
    uint16_t _pad;
    int32_t dir_y;       /* y component (default 0).  (dir, dir_y) = integer
                            baseline direction of an array pair, |comp| <= 255:
                            disparity s = dmin+d counts pixels along the major
                            axis, the minor offset is round_half_up(s*m/M)
                            (DESIGN.md §2.2); (+-1,0), (0,+-1), (+-1,+-1) are the
                            horizontal / vertical / 45-degree cases              */
} sva_sgm_params;

/* One stereo pair for the batch API. */
typedef struct sva_pair_job {
    const uint8_t* left;  /* host, reference image                  */
    const uint8_t* right; /* host, matched image                    */
    int32_t width, height;
    size_t pitch;
    uint16_t* disp;       /* host, width*height                     */
    float* subpix;        /* host, width*height or NULL             */
} sva_pair_job;

/* ------------------------------------------------------------ context --- */
void sva_sgm_params_default(sva_sgm_params* p);
int sva_abi_version(void);
int sva_device_count(int* count);
int sva_create(int device, void** ctx_out);          /* sva_ctx* as void*   */
int sva_destroy(void* ctx);
/* Adopt an external hipStream_t (NULL = the context's own stream). */
int sva_set_stream(void* ctx, void* hip_stream);
int sva_synchronize(void* ctx);
const char* sva_last_error(void* ctx);
const char* sva_status_string(int status);
/* Pre-size the workspace for W x H x D (optional; calls grow it on demand).
 * When the frame's stage buffers (cost volume, diagonal path volumes,
 * checkpoints) reach 4 GiB, reserve also checks their placement: it times the
 * path kernel on the buffers it got and on up to five further allocations of
 * them (all held until it chooses, while a quarter of the device memory stays
 * free), keeps the fastest set and frees the others (at 4K
 * D=256 the kernel's rate depends on which physical pages the 10.6 GB of
 * volumes land on, 4.3-4.9 ms, and not on anything else measured).  About
 * 0.2 s at 4K D=256, once per allocation; the call then returns after the
 * trial launches have finished on the context stream (work queued on that
 * stream before it runs first).  SVA_DEBUG_PLACEMENT_TRIALS sets the count
 * (1 = off). */
int sva_reserve(void* ctx, int width, int height, int D);

/* Path-aggregation route of sva_disparity_sgm*.  COST_VOLUME (= AUTO, the
 * default): census -> W*H*D u8 cost volume -> 8-path kernel writing the four
 * diagonal volumes and the horizontal / vertical checkpoints -> per-tile
 * recompute of those four directions + WTA (the tile pipeline, DESIGN.md
 * §4.9).  FUSED (the
 * census-fused path kernel of ABI v1-v3, slower at every D once the
 * checkpoint route existed) was removed in ABI v4: selecting it returns
 * SVA_ERR_UNSUPPORTED. */
#define SVA_PATH_KERNEL_COST_VOLUME 0
#define SVA_PATH_KERNEL_FUSED 1
#define SVA_PATH_KERNEL_AUTO 2
int sva_set_path_kernel(void* ctx, int kernel);

/* Kernel timing with hipEvents on the context stream (measurement only).
 * enable: SVA_TIMING_OFF, SVA_TIMING_ALL (every launch), SVA_TIMING_PATHS
 * (only the path-aggregation launch "sgm_paths") or SVA_TIMING_AGG
 * ("sgm_paths" and "wta_hv", the two kernels of the aggregation).  The
 * aggregation kernels are timed by their own dispatch's start/stop events;
 * each timed launch still costs a few microseconds of stream time. */
#define SVA_TIMING_OFF 0
#define SVA_TIMING_ALL 1
#define SVA_TIMING_PATHS 2
#define SVA_TIMING_AGG 3
int sva_set_timing(void* ctx, int enable);
int sva_reset_timing(void* ctx);
/* Total milliseconds and launch count of kernel `name` since the last reset. */
int sva_kernel_time(void* ctx, const char* name, double* total_ms, int64_t* count);

/* Per-context test and debug switches (ABI v6; they replace the round-5
 * SVA_PLANE_SPLIT environment variable, so the environment never changes
 * how production work is dispatched).  Every key defaults to 0 = off.
 *   SVA_DEBUG_PLANE_SPLIT    set: split every Mode R tile into 1..16 workgroup
 *                            shares (0 = the automatic count, ref_plan.h
 *                            plane_shares), so the parity tests cover every
 *                            share count at every size.
 *   SVA_DEBUG_FAIL_COST_AT   set: the next sva_disparity_sgm_batch_d or
 *                            sva_disparity_sgm_batch_conf_d call fails its
 *                            n-th cost launch (1-based) with SVA_ERR_DEVICE,
 *                            without launching it.  That call resets the
 *                            switch to 0 whatever its outcome, also when it
 *                            refuses its arguments (fault injection for the
 *                            side-stream join test).
 *   SVA_DEBUG_SIDE_IDLE      get: 1 if every side stream of the batch route
 *                            has finished its queued work (hipStreamQuery),
 *                            else 0.
 *   SVA_DEBUG_PLACEMENT_TRIALS  set: buffer sets sva_reserve's placement check
 *                            times (1..8; 1 = no check; 0 = the default, 6).
 *   SVA_DEBUG_PLACEMENT_NS   get: the path kernel's time on the set the last
 *                            check kept, ns (0: no check ran).
 *   SVA_DEBUG_PLACEMENT_WORST_NS  get: the slowest set that check timed, ns.
 *   SVA_DEBUG_DIAG_ROUTE     get: how the last single-frame aggregation carried
 *                            its four diagonal directions: 0 = four L_r
 *                            volumes, 1 = two pair-sum volumes (the pair
 *                            route: native D = 128 with 2 * P2 <= 255, frames
 *                            of at least the threshold below).
 *   SVA_DEBUG_DIAG_PAIR_MIN_PIXELS  set / get: the smallest frame (W * H) that
 *                            takes the pair route; -1 restores the built-in
 *                            threshold (small frames are faster on four
 *                            volumes), 0 lets the parity tests run the pair
 *                            route at every size.
 *   SVA_DEBUG_REFINE_ROUTE   set / get: 0 = sva_improve_with_disparity* picks
 *                            its kernel by k (below), 1 = the box-sum route
 *                            for every k >= 1, so the parity tests can run it
 *                            where the two small-window kernels are witnesses.
 *   SVA_DEBUG_REFINE_LAST_ROUTE  get: the kernel of the last refinement launch:
 *                            0 = refine_box_kernel (k 1..16), 1 =
 *                            refine_kernel (k 0; k 1..16 on planes of 2^31
 *                            bytes or more), 2 = the box-sum route
 *                            (k >= 17), -1 = none yet.
 *   SVA_DEBUG_CROSS_ORDER    set / get: the block order of sva_cross_check*'s
 *                            kernel, 0 = view-major, 1 = tile-major, -1 restores
 *                            the built-in choice (get returns the order in
 *                            force).  Speed only: the outputs do not change.
 *   SVA_DEBUG_FILL_SEGMENT   set / get: the segment length of sva_fill_holes*'s
 *                            scan, 1..65536; 0 restores the built-in length
 *                            (get returns the length in force).  Speed only. */
#define SVA_DEBUG_PLANE_SPLIT 1
#define SVA_DEBUG_FAIL_COST_AT 2
#define SVA_DEBUG_SIDE_IDLE 3
#define SVA_DEBUG_PLACEMENT_TRIALS 4
#define SVA_DEBUG_PLACEMENT_NS 5
#define SVA_DEBUG_PLACEMENT_WORST_NS 6
#define SVA_DEBUG_DIAG_ROUTE 7
#define SVA_DEBUG_DIAG_PAIR_MIN_PIXELS 8
#define SVA_DEBUG_REFINE_ROUTE 9
#define SVA_DEBUG_REFINE_LAST_ROUTE 10
#define SVA_DEBUG_CROSS_ORDER 11
#define SVA_DEBUG_FILL_SEGMENT 12
int sva_set_debug(void* ctx, int key, int64_t value);
int sva_get_debug(void* ctx, int key, int64_t* value);

/* ------------------------------------------------------ Mode S (SGM) --- */
/* Whole path: census -> Hamming cost -> 8-path SGM -> WTA (+ sub-pixel).
 * Replaces the inline hot loop CameraStereoVision.cpp:44-95 with the
 * north_star SGM matcher.  disp: W*H u16 (dmin + d*); subpix: W*H f32 or NULL.
 * Size limits (SVA_ERR_UNSUPPORTED beyond them): H <= 65535, and W*H*Dn < 2^32
 * where Dn is D rounded up to 64, 128, 192 or 256 -- every volume is addressed
 * with 32-bit byte offsets (e.g. 4K at D = 256 is 2.1e9, within the limit;
 * 8K x 4K at D = 256 is not). */
int sva_disparity_sgm(void* ctx, const uint8_t* left, const uint8_t* right, int width,
                      int height, size_t pitch, const sva_sgm_params* p, uint16_t* disp,
                      float* subpix);
int sva_disparity_sgm_d(void* ctx, const uint8_t* left, const uint8_t* right, int width,
                        int height, size_t pitch, const sva_sgm_params* p, uint16_t* disp,
                        float* subpix);

/* The same frame with the WTA's confidence.  cost_min: W*H
 * u16, S(d*), the 8-path sum at the winning disparity; cost_second: W*H u16,
 * the smallest S(d) over the caller's disparities with |d - d*| > 1, 0xFFFF
 * when there is none (D <= 3).  Either plane may be NULL.  uniqueness = u in
 * 0..100 (SVA_ERR_INVALID_ARG outside), 0 = off: a pixel with a cost_second
 * and cost_second * (100 - u) < cost_min * 100 gets disp = p->invalid and
 * subpix = NaN (the marks of lr_check); the cost planes keep their values.
 * With lr_check the reference map is filtered first and a pixel is invalid if
 * either test rejects it; the planes come from the reference pass.  With
 * uniqueness = 0 the disp / subpix output equals sva_disparity_sgm*'s. */
int sva_disparity_sgm_conf(void* ctx, const uint8_t* left, const uint8_t* right, int width,
                           int height, size_t pitch, const sva_sgm_params* p, int uniqueness,
                           uint16_t* disp, float* subpix, uint16_t* cost_min,
                           uint16_t* cost_second);
int sva_disparity_sgm_conf_d(void* ctx, const uint8_t* left, const uint8_t* right, int width,
                             int height, size_t pitch, const sva_sgm_params* p, int uniqueness,
                             uint16_t* disp, float* subpix, uint16_t* cost_min,
                             uint16_t* cost_second);

/* Multi-baseline Mode S: ONE reference image against n
 * matched images (1 <= n <= 32), image i along its own step steps[i] = (dir,
 * dir_y) (steps: host [n][2] i32; p->dir and p->dir_y are ignored).  The n
 * pairs' cost volumes are fused before the aggregation -- per pixel and
 * disparity the mean, rounded half up, over the pairs whose matched pixel lies
 * inside the image, 62 where none does -- and one 8-path SGM + WTA runs on the
 * fused volume.  The same disparity must mean the same depth in every pair:
 * pairs whose baselines share their major-axis component (all 8 neighbours of a
 * camera).  n = 1 equals sva_disparity_sgm_conf* of that pair;
 * the result does not depend on the order of the images.  others: host array of
 * n image pointers (device images for _d, host images otherwise).  The outputs,
 * uniqueness and the size limits are those of sva_disparity_sgm_conf*; the
 * confidence planes are optional.  Any D in 1..256.  lr_check has no multi-view
 * definition: SVA_ERR_UNSUPPORTED (the consistency test between several
 * reference cameras' maps is sva_cross_check*, below).  n outside 1..32, a null image or a zero
 * step: SVA_ERR_INVALID_ARG, before anything is launched.
 * Workspace: the context's cost workspace grows to (n + 1) * W * H * Dn bytes
 * (Dn = D rounded up to 64, 128, 192 or 256; 2.4 GB for n = 8 at 1080p D = 128)
 * next to the aggregation's own volumes, and stays allocated. */
int sva_disparity_sgm_multi(void* ctx, const uint8_t* ref, const uint8_t* const* others,
                            const int32_t* steps, int n, int width, int height, size_t pitch,
                            const sva_sgm_params* p, int uniqueness, uint16_t* disp,
                            float* subpix, uint16_t* cost_min, uint16_t* cost_second);
int sva_disparity_sgm_multi_d(void* ctx, const uint8_t* ref, const uint8_t* const* others,
                              const int32_t* steps, int n, int width, int height, size_t pitch,
                              const sva_sgm_params* p, int uniqueness, uint16_t* disp,
                              float* subpix, uint16_t* cost_min, uint16_t* cost_second);
/* The fusion stage alone: n device volumes [H][W][D] u8, volume i at volumes +
 * i * stride (stride in bytes, >= W*H*D, may exceed 2^32), into fused
 * [H][W][D].  D native (64, 128, 192, 256; SVA_ERR_UNSUPPORTED otherwise);
 * dreal in 1..D: fused = 255 at d >= dreal.  Any u8 input
 * values are accepted.  volumes, stride and fused must be multiples of 16
 * (SVA_ERR_INVALID_ARG). */
int sva_cost_fuse_d(void* ctx, const uint8_t* volumes, size_t stride, int n, int width,
                    int height, int D, int dreal, int dmin, const int32_t* steps,
                    uint8_t* fused);

/* Mixed-baseline Mode S: sva_disparity_sgm_multi* for pairs
 * of UNEQUAL baselines.  The group has one unit baseline; disparity s = dmin +
 * d counts major-axis pixels of a pair whose baseline is that unit, and depth
 * is unit_baseline * f / (d * pixel_size).  Pair i's major-axis baseline is
 * ratios[i] = (num, den) times the unit (ratios: host [n][2] i32, each in 1..8,
 * reduced by their gcd on entry): it matches pixel p at disparity s against
 * p + off_i(t), t = (2*s*num + den) / (2*den) -- s*num/den rounded half up --
 * with off_i the offset of its step, costs 62 where that pixel leaves the
 * image, and is visible in the fusion exactly there.  Fusion, aggregation, WTA,
 * confidence and uniqueness are those of sva_disparity_sgm_multi*, and with
 * every ratio 1/1 so is every output byte.  The result does not depend on the
 * order of the pairs.  A pair at 1/1 takes the frame's own cost kernels; every
 * other pair costs one census launch and one cost_mixed launch.
 * Refused before anything is launched: null ratios, num or den outside 1..8, a
 * match distance t(dmin + D - 1) above 65535 (SVA_ERR_INVALID_ARG), and
 * everything sva_disparity_sgm_multi* refuses (lr_check: SVA_ERR_UNSUPPORTED;
 * sva_cross_check* is the multi-view consistency test).
 * Workspace as for sva_disparity_sgm_multi*, plus two census maps (16 bytes per
 * pixel). */
int sva_disparity_sgm_mixed(void* ctx, const uint8_t* ref, const uint8_t* const* others,
                            const int32_t* steps, const int32_t* ratios, int n, int width,
                            int height, size_t pitch, const sva_sgm_params* p, int uniqueness,
                            uint16_t* disp, float* subpix, uint16_t* cost_min,
                            uint16_t* cost_second);
int sva_disparity_sgm_mixed_d(void* ctx, const uint8_t* ref, const uint8_t* const* others,
                              const int32_t* steps, const int32_t* ratios, int n, int width,
                              int height, size_t pitch, const sva_sgm_params* p, int uniqueness,
                              uint16_t* disp, float* subpix, uint16_t* cost_min,
                              uint16_t* cost_second);
/* The cost stage of one such pair from two device census maps (sva_census_d):
 * C[(y*W + x)*D + d] = popcount(census_ref(p) ^ census_oth(p + off(t(dmin +
 * d)))) along the step (sx, sy) at ratio num/den, 62 outside the image, 255 at
 * d >= dreal.  D native, dreal, dmin and the size limit as for sva_cost_fuse_d;
 * C must be a multiple of 16, the maps of 8. */
int sva_cost_mixed_d(void* ctx, const uint64_t* census_ref, const uint64_t* census_oth, int width,
                     int height, int D, int dreal, int dmin, int sx, int sy, int num, int den,
                     uint8_t* C);
/* sva_cost_fuse_d with the visibility rule of §2.2d: volume i belongs to a pair
 * at ratios[i] = (num, den) (host [n][2] i32, each in 1..8).  All ratios 1/1:
 * the bytes of sva_cost_fuse_d. */
int sva_cost_fuse_mixed_d(void* ctx, const uint8_t* volumes, size_t stride, int n, int width,
                          int height, int D, int dreal, int dmin, const int32_t* steps,
                          const int32_t* ratios, uint8_t* fused);

/* A batch of device-resident frames of one shape on this context's stream:
 * pair j matches jobs[j].left against jobs[j].right along its own step
 * (params.dir, params.dir_y), and every frame's cost volume then goes through
 * ONE sgm_paths and ONE wta_hv launch (up to 8 frames per launch), so small
 * frames fill the chip (the reference's half-size renders,
 * CameraStereoVision.cpp:17-18, at the pair loop of :55).  The jobs must share
 * D, dmin, P1, P2 and subpixel (SVA_ERR_INVALID_ARG otherwise) and may not set
 * lr_check (SVA_ERR_UNSUPPORTED).  maps: [n][H][W] u16 device; subpix:
 * [n][H][W] f32 device or NULL.  Results equal sva_disparity_sgm_d per pair.
 * sva_pair_d is declared with the multi-GPU engine below. */
struct sva_pair_d;
int sva_disparity_sgm_batch_d(void* ctx, const struct sva_pair_d* jobs, int n_jobs, int width,
                              int height, size_t pitch, uint16_t* maps, float* subpix);
/* The same batch through wta_hv's confidence instance (DESIGN.md §2.4b,
 * §4.10): frame j's maps / subpix / cost_min / cost_second planes equal
 * sva_disparity_sgm_conf_d's for that pair byte for byte.  cost_min,
 * cost_second: [n][H][W] u16 device, each may be NULL.  The rules of
 * sva_disparity_sgm_batch_d hold (lr_check: SVA_ERR_UNSUPPORTED); the jobs
 * must also share params.invalid, and uniqueness must lie in 0..100
 * (SVA_ERR_INVALID_ARG).  With uniqueness = 0, maps / subpix equal
 * sva_disparity_sgm_batch_d's. */
int sva_disparity_sgm_batch_conf_d(void* ctx, const struct sva_pair_d* jobs, int n_jobs,
                                   int width, int height, size_t pitch, int uniqueness,
                                   uint16_t* maps, float* subpix, uint16_t* cost_min,
                                   uint16_t* cost_second);

/* Stage entry points (device buffers).  Layouts: census W*H u64; C, L
 * [y][x][d] u8; S [y][x][d] u16; L volumes [8][y][x][d] (direction table in
 * DESIGN.md §2.3).  Each buffer must hold exactly its documented shape for
 * the (width, height, D) passed; the tile stages below take byte sizes. */
int sva_census_d(void* ctx, const uint8_t* img, int width, int height, size_t pitch,
                 uint64_t* census);
int sva_cost_d(void* ctx, const uint64_t* census_l, const uint64_t* census_r, int width,
               int height, const sva_sgm_params* p, uint8_t* C);
/* Census of both images and the cost volume in one kernel, the one
 * sva_disparity_sgm* runs: 1-D steps (dir_y = 0), and 2-D steps whose
 * primitive form has |dir_y| = 1 and |dir| <= 3 (every baseline of the
 * reference's 5x5 rig, functions.cpp:148-213, and of a 2x4 grid); other
 * steps return SVA_ERR_UNSUPPORTED.  Same C bytes as sva_census_d x2 ->
 * sva_cost_d; the census maps stay on chip. */
int sva_census_cost_d(void* ctx, const uint8_t* left, const uint8_t* right, int width,
                      int height, size_t pitch, const sva_sgm_params* p, uint8_t* C);
int sva_paths_d(void* ctx, const uint8_t* C, int width, int height, const sva_sgm_params* p,
                uint8_t* L8);
int sva_aggregate_d(void* ctx, const uint8_t* C, int width, int height,
                    const sva_sgm_params* p, uint16_t* S);
/* The two stages of the frame route, the tile pipeline (DESIGN.md §4.9,
 * §4.11).
 *   sva_paths_tile_d: diag = [diag_volumes][H][W][D] u8, the diagonal
 *     volumes (diag_volumes = 4 in this build: directions 4..7, the values of
 *     those slots of sva_paths_d); hckpt = [2][H][nsx][D] u8, hckpt[0][y][s]
 *     = L_0(s*seg + seg - 1, y) and hckpt[1][y][s] = L_1(s*seg, y); vckpt =
 *     [6 - diag_volumes][nsy][W][D] u8, vckpt[0][s][x] = L_2(x, s*seg + seg
 *     - 1), vckpt[1][s][x] = L_3(x, s*seg) (entries with no such column / row
 *     are not written).  Experiment builds that recompute diagonals per tile
 *     (measured slower and not shipped) report
 *     diag_volumes 2 or 0 and carry those diagonals' row checkpoints in
 *     vckpt planes 2.. instead; size every buffer from sva_tile_layout_of.
 *   sva_wta_hv_d: recomputes the checkpointed directions per 16 x seg tile,
 *     sums S with the diagonal volumes, picks d* (+ sub-pixel).
 * Every buffer comes with its size in bytes: a buffer smaller than its plane
 * returns SVA_ERR_INVALID_ARG before anything is launched.  seg, nsx, nsy and
 * the plane sizes come from sva_tile_layout_of (no device needed);
 * sva_tile_check applies the entry points' size test alone. */
typedef struct sva_tile_layout {
    int32_t seg;          /* checkpoint spacing, columns and rows            */
    int32_t nsx, nsy;     /* ceil(W / seg), ceil(H / seg)                    */
    int32_t diag_volumes; /* 4: directions 4..7 (2 or 0: §4.11 builds)     */
    size_t cost_bytes;    /* C      [H][W][D]                                */
    size_t diag_bytes;    /* diag   [diag_volumes][H][W][D]                  */
    size_t hckpt_bytes;   /* hckpt  [2][H][nsx][D]                           */
    size_t vckpt_bytes;   /* vckpt  [6 - diag_volumes][nsy][W][D]            */
} sva_tile_layout;
int sva_tile_layout_of(int width, int height, int D, sva_tile_layout* out);
int sva_tile_check(int width, int height, int D, size_t C_bytes, size_t diag_bytes,
                   size_t hckpt_bytes, size_t vckpt_bytes);
int sva_paths_tile_d(void* ctx, const uint8_t* C, size_t C_bytes, int width, int height,
                     const sva_sgm_params* p, uint8_t* diag, size_t diag_bytes, uint8_t* hckpt,
                     size_t hckpt_bytes, uint8_t* vckpt, size_t vckpt_bytes);
int sva_wta_hv_d(void* ctx, const uint8_t* C, size_t C_bytes, const uint8_t* diag,
                 size_t diag_bytes, const uint8_t* hckpt, size_t hckpt_bytes,
                 const uint8_t* vckpt, size_t vckpt_bytes, int width, int height,
                 const sva_sgm_params* p, uint16_t* disp, float* subpix);
/* The same two stages on the plan a whole frame runs: what
 * sva_disparity_sgm* launches after its cost kernel, on the caller's buffers
 * in place of the context's two workspaces.  The route is the frame's own:
 * two pair-sum volumes (§4.15) where the D class has them, 2 * P2 fits a u8
 * and width * height reaches the pixel threshold, else four volumes; minima
 * planes (§4.17) where the D class has them.
 *   D: the volumes have the native width layout.D = 64, 128, 192 or 256, the
 *     smallest that holds p->D (the other stage entries take that width as
 *     p->D; here p->D in 1..256 is the caller's disparity count, as for whole
 *     frames, and C holds 255 at d >= p->D, as sva_census_cost_d's padded
 *     frames and sva_cost_fuse_d's dreal do, §4.7).
 *   sva_frame_layout_of (no device needed): the plan of this shape and these
 *     penalties.  pair_min_pixels = -1: the built-in threshold; the two
 *     entries use the context's (SVA_DEBUG_DIAG_PAIR_MIN_PIXELS or built in).
 *   volumes = [n_volumes][H][W][D] u8.  route 0: L_4 .. L_7.  route 1:
 *     E_0 = (L_4 - C) + (L_5 - C), E_1 = (L_6 - C) + (L_7 - C).
 *   ckpt, one buffer of ckpt_bytes; at
 *     hck_off: [2][H][nsx][D], as hckpt above;
 *     vck_off: [2][nsy][W][D], as vckpt above;
 *     pair_off (route 1): [2][nsy][W][D], plane j of the pair 4+5 (j = 0) or
 *       6+7 (j = 1).  With q = (nsy / 2): row s < q - 1 holds
 *       L_{4+2j}(x, s*seg + seg - 1), row s > q holds L_{5+2j}(x, s*seg); rows
 *       q - 1 and q are not written (those states stay in registers, §4.16);
 *     hmn_off (minima): [2][H][nsx][8], vmn_off: [2][nsy][W][8]: the minimum
 *       each step of directions 0, 1 / 2, 3 entered with, 0 at a line's first
 *       pixel, else min_k L_r of the line's previous pixel.  Byte i of a
 *       segment is its pixel i (directions 0, 2) or 7 - i (directions 1, 3);
 *       bytes of pixels outside the image have no meaning.
 *     At d >= p->D the volumes and checkpoints have no meaning.
 *   sva_wta_frame_d: cost_min = cost_second = NULL and uniqueness = 0 run the
 *     plain instance; anything else the confidence instance, by the rule of
 *     sva_disparity_sgm_conf_d.  subpix is written when p->subpixel is set.
 * A buffer smaller than the layout's size is SVA_ERR_INVALID_ARG before
 * anything is launched. */
typedef struct sva_frame_layout {
    int32_t route;        /* 0 four volumes, 1 pair sums (SVA_DEBUG_DIAG_ROUTE) */
    int32_t minima;       /* 1: hmn / vmn exist                                */
    int32_t D;            /* native width of every [..][D] plane               */
    int32_t seg, nsx, nsy;
    int32_t n_volumes;    /* 4 or 2                                            */
    int32_t reserved;
    size_t cost_bytes;    /* C [H][W][D], also one route volume                */
    size_t volumes_bytes; /* n_volumes * cost_bytes                            */
    size_t ckpt_bytes;
    size_t hck_off, hck_bytes;
    size_t vck_off, vck_bytes;
    size_t pair_off, pair_bytes;   /* bytes 0 on route 0                       */
    size_t hmn_off, hmn_bytes;     /* bytes 0 without minima                   */
    size_t vmn_off, vmn_bytes;
} sva_frame_layout;
int sva_frame_layout_of(int width, int height, const sva_sgm_params* p, long long pair_min_pixels,
                        sva_frame_layout* out);
int sva_paths_frame_d(void* ctx, const uint8_t* C, size_t C_bytes, int width, int height,
                      const sva_sgm_params* p, uint8_t* volumes, size_t volumes_bytes,
                      uint8_t* ckpt, size_t ckpt_bytes);
int sva_wta_frame_d(void* ctx, const uint8_t* C, size_t C_bytes, const uint8_t* volumes,
                    size_t volumes_bytes, const uint8_t* ckpt, size_t ckpt_bytes, int width,
                    int height, const sva_sgm_params* p, int uniqueness, uint16_t* disp,
                    float* subpix, uint16_t* cost_min, uint16_t* cost_second);
int sva_wta_d(void* ctx, const uint16_t* S, int width, int height, const sva_sgm_params* p,
              uint16_t* disp, float* subpix);
/* sva_wta_d with the confidence planes and the uniqueness filter of
 * sva_disparity_sgm_conf_d (cost_min, cost_second nullable). */
int sva_wta_conf_d(void* ctx, const uint16_t* S, int width, int height, const sva_sgm_params* p,
                   int uniqueness, uint16_t* disp, float* subpix, uint16_t* cost_min,
                   uint16_t* cost_second);

/* -------------------------------------------- Mode R (reference parity) --- */
/* The reference's own path, bit-exact: per pixel the t_near/t_far ray ends
 * (CameraStereoVision.cpp:60-64, Camera.cpp:15-34), bounds check (:66-71),
 * Bresenham candidates (functions.cpp:253-321), 2k x 2k SAD (getAbsDiff,
 * functions.cpp:215-218), first-minimum WTA (:85), (uchar)(int)norm (:89).
 * mask: W*H u8 or NULL (all selected, :53).  Writes only pixels the pair keeps
 * (multi-pair callers overwrite in order, :55); disp_u16 / valid nullable.
 * The context keeps a W*H key buffer (u32; u64 when a line can hold 4,096
 * or more candidates, i.e. W or H >= 4096; grown on demand, freed by
 * sva_destroy) where a tile's workgroups merge their first minima.
 * Limits: 1 <= k, 2k < W and 2k < H (the reference's own window bounds,
 * CameraStereoVision.cpp:49-51); W, H <= 32767.  k <= 32 runs the
 * offset-plane kernel, larger k one wave per pixel. */
int sva_disparity_ref(void* ctx, const uint8_t* ref_img, const uint8_t* other_img, int width,
                      int height, size_t pitch, const uint8_t* mask,
                      const sva_camera* ref_cam, const sva_camera* other_cam, int k,
                      double t_near, double t_far, uint8_t* disp_u8, uint16_t* disp_u16,
                      uint8_t* valid);
int sva_disparity_ref_d(void* ctx, const uint8_t* ref_img, const uint8_t* other_img,
                        int width, int height, size_t pitch, const uint8_t* mask,
                        const sva_camera* ref_cam, const sva_camera* other_cam, int k,
                        double t_near, double t_far, uint8_t* disp_u8, uint16_t* disp_u16,
                        uint8_t* valid);
/* Stage: per-pixel ray endpoints (CameraStereoVision.cpp:60-71).
 * ends: W*H*4 int32 (p1x, p1y, p2x, p2y); valid: W*H u8. */
int sva_ref_endpoints_d(void* ctx, int width, int height, const sva_camera* ref_cam,
                        const sva_camera* other_cam, int k, double t_near, double t_far,
                        int32_t* ends, uint8_t* valid);

/* ---------------------- refinement and 3-D output --
 * Semantics of the reference's undefined corners: DESIGN.md §2.7.  Every
 * u8 plane of a call shares `pitch`; depth planes are dense W*H f64.  Pixels a
 * routine does not write keep the caller's buffer contents (the reference
 * leaves them uninitialised). */

/* shiftPerspectiveWithDisparity (functions.cpp:55-77): shifted(x, y) =
 * image((int)(d*preX + x), (int)(d*preY + y)) for d = disparity(x, y) != 0,
 * pre = (in.pos - out.pos) / |in.pos - out.pos|. */
int sva_shift_perspective_d(void* ctx, const sva_camera* in_cam, const sva_camera* out_cam,
                            const uint8_t* disparity, const uint8_t* image, int width, int height,
                            size_t pitch, uint8_t* shifted);
int sva_shift_perspective(void* ctx, const sva_camera* in_cam, const sva_camera* out_cam,
                          const uint8_t* disparity, const uint8_t* image, int width, int height,
                          size_t pitch, uint8_t* shifted);

/* improveWithDisparity (functions.cpp:11-52): for each pair i (cam_pairs[2i],
 * cam_pairs[2i+1], paired image images[i]) shift the image by the disparity,
 * then re-search 11 candidates along the 0/1 direction with 2k x 2k SADs,
 * k = (window_size-1)/2, any window_size >= 1; the last pair wins.  k >= 17
 * runs on summed-area tables of the 11 absolute-difference planes, whose work
 * per pixel does not depend on k.  They live in a context workspace that
 * grows on demand and is freed by sva_destroy:
 *   e = 4 for k <= 2052 (32-bit sums are exact), else 8;
 *   table = e * (width + 1) * (height + 1) bytes per candidate;
 *   G = min(11, max(1, floor(512 MiB / table))) tables at a time;
 *   workspace = 256 + G * table (+ up to 7 of alignment)
 *               + (G < 11 ? 9 * width * height : 0) bytes;
 * none of it when no window fits the image.  mask nullable (= the
 * reference's getFaceMask, :13).  strict: fail with SVA_ERR_INVALID_ARG if a
 * masked pixel's window leaves the image (the reference's ROI throws);
 * otherwise such pixels are skipped.  _d: images is a HOST array of device
 * pointers; the host form takes host pointers. */
int sva_improve_with_disparity_d(void* ctx, const uint8_t* disparity, const uint8_t* center,
                                 const uint8_t* const* images, const sva_camera* cam_pairs,
                                 int n_pairs, int width, int height, size_t pitch,
                                 const uint8_t* mask, int window_size, int strict, uint8_t* out);
int sva_improve_with_disparity(void* ctx, const uint8_t* disparity, const uint8_t* center,
                               const uint8_t* const* images, const sva_camera* cam_pairs,
                               int n_pairs, int width, int height, size_t pitch,
                               const uint8_t* mask, int window_size, int strict, uint8_t* out);

/* shiftPerspective2 (functions.cpp:79-103): depth >= 0.5 scattered to
 * (x + (int)(preX/depth), y + (int)(preY/depth)), pre = (in.pos - out.pos)*f/ps;
 * collisions resolve to the last write of the reference's x-major loop. */
int sva_shift_perspective2_d(void* ctx, const sva_camera* in_cam, const sva_camera* out_cam,
                             const double* depth, int width, int height, double* shifted);
int sva_shift_perspective2(void* ctx, const sva_camera* in_cam, const sva_camera* out_cam,
                           const double* depth, int width, int height, double* shifted);

/* Points3DToDepthMap (functions.cpp:118-132): points [n][3] f64 projected
 * with Camera::project + W/2, H/2; depth = z - cam.z; the last point wins. */
int sva_points_to_depth_d(void* ctx, const double* points, int64_t n_points,
                          const sva_camera* cam, int width, int height, double* depth);
int sva_points_to_depth(void* ctx, const double* points, int64_t n_points,
                        const sva_camera* cam, int width, int height, double* depth);

/* DepthMapToPoints3D (functions.cpp:134-146): every pixel with depth > 0.1,
 * in the reference's column-major order, to pos + inv_project(pixel - half)
 * * depth.  points: capacity width*height*3 f64; *n_points (host) = count. */
int sva_depth_to_points_d(void* ctx, const double* depth, int width, int height,
                          const sva_camera* cam, double* points, int64_t* n_points);
int sva_depth_to_points(void* ctx, const double* depth, int width, int height,
                        const sva_camera* cam, double* points, int64_t* n_points);

/* ------------------------------------------ ingestion --
 * resize(img, img, Size(), 0.5, 0.5) with the default INTER_LINEAR
 * (CameraStereoVision.cpp:18): OpenCV 4.2's exact-2x area path -- output
 * (cvRound(W/2), cvRound(H/2)) (half to even), full 2x2 blocks
 * (sum + 2) >> 2, partial edge blocks cvRound(sum / count).  u8 planes. */
int sva_resize_half_size(int width, int height, int* out_width, int* out_height);
int sva_resize_half_d(void* ctx, const uint8_t* src, int width, int height, size_t pitch,
                      uint8_t* dst, size_t dst_pitch);
int sva_resize_half(void* ctx, const uint8_t* src, int width, int height, size_t pitch,
                    uint8_t* dst, size_t dst_pitch);

/* ------------------------------------------ evaluation --
 * The reference's ground-truth comparison (CameraStereoVision.cpp:107-110,
 * 118-119) and calculateAverageError (functions.cpp:348-354), on dense
 * row-major f64 matrices.  OpenCV 4.2 semantics restated (DESIGN.md §2.8;
 * OpenCV absent: parity unpinned):
 *   sva_resize_linear_f64: resize(src, dst, Size(dw, dh)), INTER_LINEAR --
 *     copy at equal size, the area path at exactly 2x, else float-coefficient
 *     bilinear taps (x clamped, y rows clipped).
 *   sva_ref_error: error = (resize(depth, ref.size()) - ref) * scale,
 *     evaluated as OpenCV's addWeighted: a * scale + b * (-scale) + 0.
 *   sva_masked_mean: cv::mean(image, mask)[0]; mask nullable (= all pixels);
 *     0 for an empty mask.  *mean is a HOST pointer in both forms (the _d form
 *     synchronises the context stream). */
int sva_resize_linear_f64_d(void* ctx, const double* src, int src_w, int src_h, double* dst,
                            int dst_w, int dst_h);
int sva_resize_linear_f64(void* ctx, const double* src, int src_w, int src_h, double* dst,
                          int dst_w, int dst_h);
int sva_ref_error_d(void* ctx, const double* depth, int width, int height, const double* ref,
                    int ref_w, int ref_h, double scale, double* error);
int sva_ref_error(void* ctx, const double* depth, int width, int height, const double* ref,
                  int ref_w, int ref_h, double scale, double* error);
int sva_masked_mean_d(void* ctx, const double* image, const uint8_t* mask, int width, int height,
                      double* mean);
int sva_masked_mean(void* ctx, const double* image, const uint8_t* mask, int width, int height,
                    double* mean);

/* Multi-pair depth fusion on the root: per
 * pixel the median of baseline_i * f / (disp_i * pixel_size) over the maps
 * with disp_i != invalid and disp_i > 0 (mean of the middle two for an even
 * count), 0 if none.  disps: [n_maps][H][W] u16 (device / host), baselines:
 * HOST array of n_maps per-axis baselines (m), n_maps <= 32; n_valid nullable. */
int sva_fuse_depth_d(void* ctx, const uint16_t* disps, int n_maps, int width, int height,
                     const double* baselines, double f, double pixel_size, uint16_t invalid,
                     double* depth, uint8_t* n_valid);
int sva_fuse_depth(void* ctx, const uint16_t* disps, int n_maps, int width, int height,
                   const double* baselines, double f, double pixel_size, uint16_t invalid,
                   double* depth, uint8_t* n_valid);

/* Cost-aware fusion (SURVEY.md §8e "or min-cost"): per pixel
 * the depth baseline_i * f / (disp_i * pixel_size) of ONE map, chosen among
 * the maps valid there (disp_i != invalid, disp_i > 0) by the confidence
 * planes of sva_disparity_sgm_conf*: SVA_FUSE_MIN_COST the smallest cost_min,
 * SVA_FUSE_MAX_MARGIN the largest cost_second - cost_min (unsigned 32-bit,
 * 0xFFFF as is); ties go to the lowest map index; 0 if no map is valid.
 * disps, cost_min, cost_second: [n_maps][H][W] u16 (cost_second may be NULL
 * for SVA_FUSE_MIN_COST); n_maps <= 32; n_valid, winner (the chosen map's
 * index, 0xFF if none) nullable.  A NULL cost_second with MAX_MARGIN, another
 * mode or n_maps outside 1..32 return SVA_ERR_INVALID_ARG. */
#define SVA_FUSE_MIN_COST 0
#define SVA_FUSE_MAX_MARGIN 1
int sva_fuse_depth_conf_d(void* ctx, const uint16_t* disps, const uint16_t* cost_min,
                          const uint16_t* cost_second, int n_maps, int width, int height,
                          const double* baselines, double f, double pixel_size, uint16_t invalid,
                          int mode, double* depth, uint8_t* n_valid, uint8_t* winner);
int sva_fuse_depth_conf(void* ctx, const uint16_t* disps, const uint16_t* cost_min,
                        const uint16_t* cost_second, int n_maps, int width, int height,
                        const double* baselines, double f, double pixel_size, uint16_t invalid,
                        int mode, double* depth, uint8_t* n_valid, uint8_t* winner);

/* Sub-pixel fusion: the four calls above with the depth of a
 * map taken from its f32 sub-pixel disparity, baseline_i * f / ((double)
 * subpix_i * pixel_size), so that depth is no longer quantised to whole
 * disparities.  subpix: [n_maps][H][W] f32 (device / host), the sub-pixel maps
 * the matchers write next to disps (NaN where a pixel was rejected).  Map i is
 * valid at a pixel where disp_i != invalid, disp_i > 0 and subpix_i > 0.0f
 * (false for NaN).  The winner of the cost-aware modes is chosen as above among
 * those maps.  Where subpix_i == (float)disp_i everywhere, every output equals
 * that of the u16 call bit for bit.  A NULL subpix returns SVA_ERR_INVALID_ARG;
 * every other rule is that of the u16 call. */
int sva_fuse_depth_sub_d(void* ctx, const uint16_t* disps, const float* subpix, int n_maps,
                         int width, int height, const double* baselines, double f,
                         double pixel_size, uint16_t invalid, double* depth, uint8_t* n_valid);
int sva_fuse_depth_sub(void* ctx, const uint16_t* disps, const float* subpix, int n_maps,
                       int width, int height, const double* baselines, double f,
                       double pixel_size, uint16_t invalid, double* depth, uint8_t* n_valid);
int sva_fuse_depth_conf_sub_d(void* ctx, const uint16_t* disps, const float* subpix,
                              const uint16_t* cost_min, const uint16_t* cost_second, int n_maps,
                              int width, int height, const double* baselines, double f,
                              double pixel_size, uint16_t invalid, int mode, double* depth,
                              uint8_t* n_valid, uint8_t* winner);
int sva_fuse_depth_conf_sub(void* ctx, const uint16_t* disps, const float* subpix,
                            const uint16_t* cost_min, const uint16_t* cost_second, int n_maps,
                            int width, int height, const double* baselines, double f,
                            double pixel_size, uint16_t invalid, int mode, double* depth,
                            uint8_t* n_valid, uint8_t* winner);

/* Cross-view consistency check between the maps of several reference cameras
 * (DESIGN.md §2.5b): the multi-view counterpart of lr_check, one pass over maps
 * that already exist.  disps: [n_views][H][W] u16 (device / host), every map
 * counting pixels of the SAME unit baseline.  view_step: HOST [n_views][2] i32,
 * each view's position in unit baselines in the sense of sva_sgm_params (dir,
 * dir_y): the match step from view a to view b is e = view_step[b] -
 * view_step[a], so view a's pixel p at disparity s lies at q = p + s * e in
 * view b, exactly.  For view a, pixel p, s = disps[a][p]:
 *   s == invalid or s == 0   out = s, agree = conflict = 0;
 *   else every b != a with q inside the image and t = disps[b][q] valid counts:
 *     |t - s| <= max_diff    agree += 1
 *     t < s - max_diff       conflict += 1 (b sees through the point)
 *     t > s + max_diff       neither (b is occluded by something nearer)
 *   out = s if agree >= min_agree and conflict <= max_conflict, else invalid.
 * subpix (nullable): [n_views][H][W] f32; out_sub (nullable, needs subpix) gets
 * subpix where the pixel is kept or was not valid and NaN where it is rejected
 * (the marks of lr_check).  agree, conflict (nullable): [n_views][H][W] u8.
 * Every view is checked against the INPUT maps.  Integer-only, so every output
 * is exact; min_agree = 0 with max_conflict = 31 copies the input.
 * SVA_ERR_INVALID_ARG, before anything is launched: n_views outside 1..32, a
 * null disps, view_step or out, a step component outside -255..255, two views
 * with equal view_step, max_diff < 0, min_agree or max_conflict outside 0..31,
 * out_sub without subpix, out or out_sub overlapping disps or subpix.
 * SVA_ERR_UNSUPPORTED: width * height >= 2^31.  _d is asynchronous on the
 * context stream; its kernel is timed as "cross_check". */
int sva_cross_check_d(void* ctx, const uint16_t* disps, const float* subpix, int n_views,
                      int width, int height, const int32_t* view_step, uint16_t invalid,
                      int max_diff, int min_agree, int max_conflict, uint16_t* out,
                      float* out_sub, uint8_t* agree, uint8_t* conflict);
int sva_cross_check(void* ctx, const uint16_t* disps, const float* subpix, int n_views, int width,
                    int height, const int32_t* view_step, uint16_t invalid, int max_diff,
                    int min_agree, int max_conflict, uint16_t* out, float* out_sub,
                    uint8_t* agree, uint8_t* conflict);

/* Speckle filter: removes the small connected components of
 * n_maps >= 1 disparity maps disps [n_maps][H][W] u16 (device / host), the
 * post-filter of OpenCV's filterSpeckles and libSGM's speckleWindowSize /
 * speckleRange, on the device.  A pixel is valid iff d != invalid and d != 0.
 * Two pixels of one map are linked iff they are 4-neighbours, both valid, and
 * |d1 - d2| <= max_diff (against the neighbour, not against a seed; max_diff
 * above 65535 counts as 65535).  comp_size(p) = the pixel count of p's connected
 * component of that graph, 0 where p is not valid; maps never connect.
 *   out = d         where p is not valid or comp_size > max_size
 *   out = invalid   where p is valid and comp_size <= max_size
 * subpix (nullable): [n_maps][H][W] f32; out_sub (nullable, needs subpix) gets
 * subpix where out = d and NaN where the pixel was removed.  comp_size
 * (nullable): [n_maps][H][W] u32.  max_size in 0..2^31-1; max_size = 0 copies
 * the input bit for bit.  Integer-only and independent of any ordering: every
 * output byte has one right value.  In place is allowed: out == disps and / or
 * out_sub == subpix, exactly.
 * Workspace: 8 * n_maps * width * height bytes of device memory per context
 * (two u32 planes per map), grown on demand, kept for later calls and freed by
 * sva_destroy; none for max_size = 0 without comp_size.
 * Returned before anything is launched, in this order: SVA_ERR_INVALID_ARG for
 * a null disps or out, n_maps < 1, a width or height < 1; SVA_ERR_UNSUPPORTED
 * for width * height >= 2^31; SVA_ERR_INVALID_ARG for max_size < 0, max_diff <
 * 0, out_sub without subpix, or any overlap of an output (out, out_sub,
 * comp_size) with an input or another output other than the two in-place forms
 * above; SVA_ERR_OUT_OF_MEMORY if the workspace cannot be had.  _d is
 * asynchronous on the context stream; its four launches are timed as
 * "speckle_label", "speckle_merge", "speckle_count" and "speckle_apply" (the
 * copy: "speckle_apply" alone). */
int sva_filter_speckles_d(void* ctx, const uint16_t* disps, const float* subpix, int n_maps,
                          int width, int height, uint16_t invalid, int max_size, int max_diff,
                          uint16_t* out, float* out_sub, uint32_t* comp_size);
int sva_filter_speckles(void* ctx, const uint16_t* disps, const float* subpix, int n_maps,
                        int width, int height, uint16_t invalid, int max_size, int max_diff,
                        uint16_t* out, float* out_sub, uint32_t* comp_size);

/* Hole filling: fills the holes of n_maps >= 1 disparity maps
 * disps [n_maps][H][W] u16 (device / host) from the nearest valid pixels, the
 * last step of an SGM post-filter chain (Hirschmueller's disparity
 * interpolation).  A pixel is valid iff d != invalid and d != 0; every other
 * pixel is a hole.  For a hole p, direction k = 0..7 -- E (+1,0), W (-1,0),
 * S (0,+1), N (0,-1), SE (+1,+1), NW (-1,-1), SW (-1,+1), NE (+1,-1) -- walks
 * p + j * r_k for j = 1..max_dist inside the frame; the first valid pixel of
 * the INPUT map is its candidate (d, j, k), j counting steps on the diagonals
 * too.  Filled pixels never serve as sources.  n = the number of directions
 * with a candidate; the candidates sorted by (d, j, k):
 *   n >= min_found: out = d of element 0 (SVA_FILL_MIN), min(1, n - 1)
 *                   (SVA_FILL_SECOND, the occlusion rule: the second lowest),
 *                   (n - 1) / 2 (SVA_FILL_MEDIAN, the lower median)
 *   n <  min_found: out = disps, unchanged (0 stays 0, invalid stays invalid)
 * and out = disps at every valid pixel.  subpix (nullable): [n_maps][H][W] f32;
 * out_sub (nullable, needs subpix) gets the 32 bits of subpix at the chosen
 * candidate's source pixel where p was filled and those of subpix[p] everywhere
 * else, NaN included.  n_found (nullable): [n_maps][H][W] u8, n at the holes,
 * filled or not, and 0 at valid pixels.  max_dist in 0..255 (SVA_FILL_MAX_DIST:
 * an occlusion band is about as wide as the disparity range, and j fits eight
 * bits of the sort key); max_dist = 0 copies the input bit for bit.  min_found
 * in 1..8.  Maps never interact.  Integer-only and independent of any ordering:
 * every output byte has one right value.  In place is allowed: out == disps and
 * / or out_sub == subpix, exactly.
 * Workspace: 32 * n_maps * width * height bytes of device memory per context
 * (eight u32 key planes per map: 32 bytes per pixel), grown on demand, kept for
 * later calls and freed by sva_destroy; none for max_dist = 0.
 * Returned before anything is launched, in this order: SVA_ERR_INVALID_ARG for
 * a null disps or out, n_maps < 1, a width or height < 1; SVA_ERR_UNSUPPORTED
 * for width * height >= 2^31; SVA_ERR_INVALID_ARG for max_dist outside 0..255,
 * min_found outside 1..8, mode outside 0..2, out_sub without subpix, or any
 * overlap of an output (out, out_sub, n_found) with an input or another output
 * other than the two in-place forms above; SVA_ERR_OUT_OF_MEMORY if the
 * workspace cannot be had.  _d is asynchronous on the context stream; its two
 * launches are timed as "fill_scan" and "fill_apply" (the copy: "fill_apply"
 * alone). */
#define SVA_FILL_MIN 0
#define SVA_FILL_SECOND 1
#define SVA_FILL_MEDIAN 2
#define SVA_FILL_MAX_DIST 255
int sva_fill_holes_d(void* ctx, const uint16_t* disps, const float* subpix, int n_maps,
                     int width, int height, uint16_t invalid, int max_dist, int min_found,
                     int mode, uint16_t* out, float* out_sub, uint8_t* n_found);
int sva_fill_holes(void* ctx, const uint16_t* disps, const float* subpix, int n_maps, int width,
                   int height, uint16_t invalid, int max_dist, int min_found, int mode,
                   uint16_t* out, float* out_sub, uint8_t* n_found);

/* Weighted median filter: edge-aware smoothing of n_maps >= 1
 * disparity maps disps [n_maps][H][W] u16 (device / host) by a guide image per
 * map, the refinement step of cost-volume filtering (Rhemann et al. 2011; Ma et
 * al. 2013).  A pixel is valid iff d != invalid and d != 0.  guides: a HOST
 * array of n_maps u8 images (device pointers for _d, host pointers for the host
 * form), rows guide_pitch >= width bytes apart; weights: a HOST array of 256
 * u16 in both forms; both are read before the call returns, and both are null
 * for the unguided filter, whose weights are all 1: the plain (2r + 1)^2 median
 * over the valid pixels.  select (nullable): [n_maps][H][W] u8.
 * Pixel p is CONSIDERED iff (select is null or select[p] != 0) and (fill != 0 or
 * p is valid).  Its CANDIDATES are the pixels q inside the frame with
 * |qx - px| <= radius and |qy - py| <= radius, p included, that are valid and
 * have weight w_q = weights[|g(p) - g(q)|] > 0; n is their number and T the sum
 * of their weights.  Sorted by (d, qy, qx) ascending, the PICK is the first
 * candidate at which 2 * (the weights summed up to and including it) >= T: the
 * lower weighted median, from one source pixel.
 *   considered and n >= min_support: out[p] = the pick's d
 *   otherwise:                       out[p] = disps[p], bit for bit
 * so fill = 1 gives a hole with enough support a value and fill = 0 leaves holes
 * as they are.  subpix (nullable): [n_maps][H][W] f32; out_sub (nullable, needs
 * subpix) gets the 32 bits of subpix at the pick's source pixel where p was
 * written and those of subpix[p] elsewhere, NaN included.  support (nullable):
 * [n_maps][H][W] u16, n at the considered pixels and 0 elsewhere.  radius in
 * 1..SVA_WMED_MAX_RADIUS, min_support in 1..961, fill in 0..1.  Maps never
 * interact; only the input map is read.  Integer-only and independent of any
 * ordering: every output byte has one right value.  In place is NOT offered:
 * the window reads neighbours that other threads would be writing.
 * No workspace on the device form; the host form stages its planes.
 * Returned before anything is launched, in this order: SVA_ERR_INVALID_ARG for
 * a null disps or out, n_maps < 1, a width or height < 1; SVA_ERR_UNSUPPORTED
 * for width * height >= 2^31; SVA_ERR_INVALID_ARG for radius outside 1..15,
 * min_support outside 1..961, fill outside 0..1, guides without weights or
 * weights without guides, a null entry in guides, guide_pitch < width, out_sub
 * without subpix, or any overlap of an output (out, out_sub, support) with an
 * input (disps, subpix, select, a guide) or with another output.  _d is
 * asynchronous on the context stream and is timed as "wmed": one launch per
 * 64 maps. */
#define SVA_WMED_MAX_RADIUS 15
int sva_weighted_median_d(void* ctx, const uint16_t* disps, const float* subpix,
                          const uint8_t* const* guides, size_t guide_pitch,
                          const uint16_t* weights, const uint8_t* select, int n_maps,
                          int width, int height, uint16_t invalid, int radius,
                          int min_support, int fill, uint16_t* out, float* out_sub,
                          uint16_t* support);
int sva_weighted_median(void* ctx, const uint16_t* disps, const float* subpix,
                        const uint8_t* const* guides, size_t guide_pitch,
                        const uint16_t* weights, const uint8_t* select, int n_maps, int width,
                        int height, uint16_t invalid, int radius, int min_support, int fill,
                        uint16_t* out, float* out_sub, uint16_t* support);

/* Rectification: n >= 1 raw views src [n][src_h][src_pitch] u8
 * warped onto the ideal grid, out [n][out_h][out_pitch] u8 (device / host); the
 * output size may differ from the source size.  views: a HOST array of n
 * sva_rectify_view in both forms, read before the call returns.  For the output
 * pixel (x, y) of a view, all in f64, every operation rounded on its own (no
 * contraction), the division IEEE, in exactly this order:
 *   w  = (h6*x + h7*y) + h8
 *   u  = ((h0*x + h1*y) + h2) / w          v  = ((h3*x + h4*y) + h5) / w
 *   if k1 == k2 == p1 == p2 == k3 == 0:    sx = u, sy = v     (no distortion step)
 *   else:
 *     xn = (u - cx) / fx                   yn = (v - cy) / fy
 *     xx = xn*xn   yy = yn*yn   xy = xn*yn   r2 = xx + yy
 *     rad = 1 + r2*(k1 + r2*(k2 + r2*k3))
 *     xd = (xn*rad + (2*p1)*xy) + p2*(r2 + 2*xx)
 *     yd = (yn*rad + p1*(r2 + 2*yy)) + (2*p2)*xy
 *     sx = xd*fx + cx                      sy = yd*fy + cy
 *   inside = w > 0 and -2^20 < sx < 2^20 and -2^20 < sy < 2^20   (false on NaN)
 *   qx = (int)rint(sx*32), qy = (int)rint(sy*32)                 (half to even; 1/32 px)
 *   X = qx >> 5, a = qx & 31, Y = qy >> 5, b = qy & 31           (arithmetic shift)
 *   taps (X,Y) (X+1,Y) (X,Y+1) (X+1,Y+1), weights (32-a)(32-b), a(32-b), (32-a)b, ab
 *   value = (sum of weight * tap + 512) >> 10
 * A tap of weight 0 is neither read nor judged; a tap of positive weight outside
 * the source [0, src_w) x [0, src_h) contributes `border`.  valid (nullable): u8
 * [n][out_h][out_pitch], 1 iff the pixel is inside and every tap of positive
 * weight lies in the source.  map (nullable): i32 [n][out_h][out_w][2], (qx, qy).
 * A pixel that is not inside: value = border, valid = 0, both map entries
 * INT32_MIN.  The rule is the engine's own: it uses OpenCV's 1/32 px grid but not
 * its coefficient tables, and parity with cv::remap is not claimed.
 * Returned before anything is launched, in this order: SVA_ERR_INVALID_ARG for a
 * null src, views or out, or n, a width or a height < 1; SVA_ERR_UNSUPPORTED for
 * a width or height above SVA_RECTIFY_MAX_SIZE; SVA_ERR_INVALID_ARG for
 * src_pitch < src_w or out_pitch < out_w; border outside 0..255; out, valid or
 * map overlapping src or each other (not an in-place filter); the first rule a
 * view breaks, view 0 first, the message naming the view: a non-finite entry of
 * h; non-finite cx or cy; fx or fy not finite or <= 0; a non-finite coefficient.
 * _d is asynchronous on the context stream and is timed as "rectify": one launch
 * per 25 views. */
typedef struct sva_rectify_view {
    double h[9];            /* row-major 3x3: rectified pixel -> undistorted raw pixel */
    double cx, cy, fx, fy;  /* raw camera: principal point and focal lengths, pixels   */
    double k1, k2, p1, p2, k3; /* Brown-Conrady coefficients, OpenCV's order           */
} sva_rectify_view;
#define SVA_RECTIFY_MAX_SIZE 32767
int sva_rectify_d(void* ctx, const uint8_t* src, int n, int src_w, int src_h, size_t src_pitch,
                  const sva_rectify_view* views, int out_w, int out_h, size_t out_pitch,
                  int border, uint8_t* out, uint8_t* valid, int32_t* map);
int sva_rectify(void* ctx, const uint8_t* src, int n, int src_w, int src_h, size_t src_pitch,
                const sva_rectify_view* views, int out_w, int out_h, size_t out_pitch, int border,
                uint8_t* out, uint8_t* valid, int32_t* map);
/* A view from a calibration, on the host alone (no context): h = K_raw . R .
 * K_ideal^-1, where R takes ideal-camera rays to raw-camera rays; cx, cy, fx, fy
 * from K_raw; dist = {k1, k2, p1, p2, k3} copied.  All matrices row-major 3x3.
 * The order of operations (csrc/rectify_math.h): K_ideal^-1 by the adjugate, each
 * cofactor a difference of two products, det = (k0*c0 + k1*c3) + k2*c6, every
 * entry cofactor / det; then M = R . K_ideal^-1 and h = K_raw . M, every entry of
 * a product ((a_i0*b_0j + a_i1*b_1j) + a_i2*b_2j); no contraction.
 * SVA_ERR_INVALID_ARG for a null pointer, non-finite input, a K_raw with skew
 * (K_raw[1] or K_raw[3] != 0) or a bottom row other than 0 0 1, or a singular
 * K_ideal; *out is written on success only. */
int sva_rectify_view_of(const double K_raw[9], const double dist[5], const double R[9],
                        const double K_ideal[9], sva_rectify_view* out);

/* Masking: n_maps >= 1 disparity maps disps [n_maps][H][W] u16
 * (device / host) take `invalid` where valid [n_maps][H][W] u8 -- one plane per
 * map, a rectified reference view's valid plane -- is 0, and stay as they are
 * elsewhere.  subpix (nullable) f32; out_sub (nullable, needs subpix) gets NaN
 * where valid is 0, as the cross-view check writes a rejected pixel, and the 32
 * bits of subpix elsewhere.  In place is allowed: out == disps, out_sub == subpix.
 * Returned before anything is launched, in this order: SVA_ERR_INVALID_ARG for a
 * null disps, valid or out, n_maps < 1, a width or height < 1;
 * SVA_ERR_UNSUPPORTED for width * height >= 2^31; SVA_ERR_INVALID_ARG for out_sub
 * without subpix, or any overlap of an output with an input or the other output
 * except exactly in place.  _d is asynchronous on the context stream and is
 * timed as "mask_maps". */
int sva_mask_maps_d(void* ctx, const uint16_t* disps, const float* subpix, int n_maps, int width,
                    int height, const uint8_t* valid, uint16_t invalid, uint16_t* out,
                    float* out_sub);
int sva_mask_maps(void* ctx, const uint16_t* disps, const float* subpix, int n_maps, int width,
                  int height, const uint8_t* valid, uint16_t invalid, uint16_t* out,
                  float* out_sub);

/* Disparity -> depth, CameraStereoVision.cpp:47,98-100 (f64; 0 where disp 0). */
int sva_disparity_to_depth_d(void* ctx, const uint8_t* disp, int n, double cam_distance,
                             double f, double pixel_size, double* depth);
int sva_disparity_to_depth(void* ctx, const uint8_t* disp, int n, double cam_distance,
                           double f, double pixel_size, double* depth);

/* -------------------------------------------------- multi-pair batch --- */
/* Independent pairs round-robin over the given contexts (one per device),
 * one host thread per context.  Replaces the `for (auto pair : pairs)` loop
 * (CameraStereoVision.cpp:55) for whole-image Mode S matching on HOST images.
 * Per context, the upload of pair j+1 and the download of pair j-1 overlap
 * the compute of pair j (pinned staging, separate copy streams).  A failing
 * pair does not stop the others: job_status (nullable, n_jobs entries)
 * receives each pair's status and the call returns the first failure. */
int sva_batch_sgm(void** ctxs, int n_ctx, const sva_pair_job* jobs, int n_jobs,
                  const sva_sgm_params* p, int* job_status);

/* ----------------------------------- multi-GPU engine --- */
/* One process drives several GPUs of a node: pairs are the shard unit (pair j
 * -> device j mod n_devices, and round-robin over that device's streams), each
 * device keeps its own cost and path volumes, and the only exchange is the
 * gather of the finished u16 disparity maps (and f32 sub-pixel maps) to
 * devices[0] over xGMI -- an RCCL grouped send/recv on a single-process
 * communicator (ncclCommInitAll, librccl loaded at sva_multi_create), or peer
 * copies with SVA_MULTI_GATHER_PEER.  north_star / BASELINE configs 4-5;
 * replaces the pair loop at CameraStereoVision.cpp:55 with the pair tables of
 * functions.cpp:148-213 (sva.hpp getCameraPairs). */
#define SVA_MULTI_GATHER_RCCL 0   /* default */
#define SVA_MULTI_GATHER_PEER 1
#define SVA_MULTI_GATHER_ALL 2    /* flag: route device 0's own maps through the
                                     gather too (exercises the exchange on one GPU) */
int sva_multi_create(const int* devices, int n_devices, int streams_per_device, int flags,
                     void** multi_out);
int sva_multi_destroy(void* multi);
/* Block until every queued batch has finished on every device. */
int sva_multi_synchronize(void* multi);
const char* sva_multi_last_error(void* multi);
/* The shard plan, a pure function (no device needed): for job j,
 * device_index[j] = j mod n_devices and context_index[j] = (j / n_devices) mod
 * streams_per_device (nullable outputs); slot_index[j] = rank of j among the
 * jobs of its context (nullable). */
int sva_multi_plan(int n_devices, int streams_per_device, int n_jobs, int32_t* device_index,
                   int32_t* context_index, int32_t* slot_index);
/* The context behind (device_index, stream_index), e.g. for sva_set_timing. */
int sva_multi_context(void* multi, int device_index, int stream_index, void** ctx_out);

/* One device-resident pair: left/right live on device
 * devices[j mod n_devices] (see sva_multi_plan), pitch in bytes. */
typedef struct sva_pair_d {
    const uint8_t* left;
    const uint8_t* right;
    sva_sgm_params params;
} sva_pair_d;
/* Every pair's Mode S map, gathered into maps (device memory on devices[0],
 * [n_jobs][H][W] u16) and, when subpix is non-NULL, the f32 maps of the jobs
 * that set params.subpixel into subpix ([n_jobs][H][W] on devices[0]; the
 * planes of the other jobs are not written).  Asynchronous: the results are
 * complete on devices[0]'s first stream (stream_index 0) once the call returns
 * SVA_OK and that stream has run; sva_multi_synchronize waits for everything.
 * Work the caller queues on that stream after a call (e.g. reading maps) is
 * ordered before the next call writes maps / subpix. */
int sva_batch_sgm_d(void* multi, const sva_pair_d* jobs, int n_jobs, int width, int height,
                    size_t pitch, uint16_t* maps, float* subpix);
/* sva_batch_sgm_d with every pair through sva_disparity_sgm_conf_d on its
 * context (so per-job invalid, lr_check and subpixel work as they do there) and
 * the confidence planes gathered with the maps: cost_min, cost_second are
 * [n_jobs][H][W] u16 on devices[0], each may be NULL.  Only the planes passed
 * non-NULL are computed into the remote jobs' slots and shipped (2 bytes per
 * pixel and pair each, next to the map's 2 and a sub-pixel job's 4).
 * uniqueness outside 0..100: SVA_ERR_INVALID_ARG.  Ordering as above, for all
 * four outputs. */
int sva_batch_sgm_conf_d(void* multi, const sva_pair_d* jobs, int n_jobs, int width, int height,
                         size_t pitch, int uniqueness, uint16_t* maps, float* subpix,
                         uint16_t* cost_min, uint16_t* cost_second);

/* A camera-array frame from HOST images: pair j matches images[pairs[j].ref]
 * against images[pairs[j].other] with its own params (the 2-D step of its
 * baseline) on device j mod n_devices; the maps are gathered to devices[0],
 * which fuses group g = pairs [group_start[g], group_start[g+1]) (one
 * reference camera, DESIGN.md §2.6, with pairs[j].baseline) into depth[g].
 * Uploads run on per-device copy streams and each pair waits only for its two
 * images, so transfers overlap compute; the fused maps download as each group
 * finishes.  depth: host [n_groups][H][W] f64; n_valid (nullable) host u8,
 * same shape; maps (nullable) host [n_pairs][H][W] u16.  Synchronous.  The
 * pairs of one group must share params.invalid (SVA_ERR_INVALID_ARG). */
typedef struct sva_array_pair {
    int32_t ref;              /* index into images[]: the reference view      */
    int32_t other;            /* index into images[]: the matched view        */
    sva_sgm_params params;    /* D, dmin, (dir, dir_y) = this pair's step     */
    double baseline;          /* major-axis baseline (m) for the fusion       */
} sva_array_pair;
int sva_array_depth(void* multi, const uint8_t* const* images, int n_images, int width,
                    int height, size_t pitch, const sva_array_pair* pairs, int n_pairs,
                    const int32_t* group_start, int n_groups, double f, double pixel_size,
                    double* depth, uint8_t* n_valid, uint16_t* maps);
/* sva_array_depth with confidence (SURVEY.md §8e "the per-pixel median or
 * min-cost"): every pair is matched with the uniqueness filter (uniqueness in
 * 0..100, 0 = off; sva_disparity_sgm_conf_d), and each group is fused by
 * `mode`: SVA_FUSE_MIN_COST / SVA_FUSE_MAX_MARGIN through
 * sva_fuse_depth_conf_d, SVA_FUSE_MEDIAN through sva_fuse_depth_d on the
 * filtered maps.  The gather ships, next to the maps, only the planes the mode
 * reads (MEDIAN none, MIN_COST cost_min, MAX_MARGIN both) and those the caller
 * asks to receive.  winner (nullable): host [n_groups][H][W] u8, the chosen
 * pair's index within its group, 0xFF if none; it must be NULL with
 * SVA_FUSE_MEDIAN.  cost_min, cost_second (nullable): host [n_pairs][H][W] u16,
 * like maps.  Another mode, uniqueness outside 0..100 or a winner with MEDIAN
 * return SVA_ERR_INVALID_ARG; everything else is as for sva_array_depth, whose
 * result MEDIAN with uniqueness = 0 equals bit for bit. */
#define SVA_FUSE_MEDIAN 2   /* sva_array_depth_conf only; sva_fuse_depth_conf* keep refusing it */
int sva_array_depth_conf(void* multi, const uint8_t* const* images, int n_images, int width,
                         int height, size_t pitch, const sva_array_pair* pairs, int n_pairs,
                         const int32_t* group_start, int n_groups, double f, double pixel_size,
                         int uniqueness, int mode, double* depth, uint8_t* n_valid,
                         uint8_t* winner, uint16_t* maps, uint16_t* cost_min,
                         uint16_t* cost_second);
/* The multi-baseline ("mb") array frame: the shard unit is
 * the GROUP.  Group g runs ONE sva_disparity_sgm_multi_d -- its reference view
 * against all its matched views, the cost volumes fused before a single
 * aggregation -- on device g mod n_devices, round-robin over that device's
 * streams; one map per group is gathered (2 bytes per pixel and group, plus 2
 * for each cost plane asked for, instead of per pair) and turned into depth by
 * sva_fuse_depth_d with n_maps = 1: baseline * f / ((double)d * pixel_size), 0
 * where d is 0 or invalid.  depth: host [n_groups][H][W] f64; maps, cost_min,
 * cost_second (each nullable): host [n_groups][H][W] u16.  uniqueness as for
 * sva_array_depth_conf.  Within a group the pairs must share ref, D, dmin, P1,
 * P2 and invalid, and their baselines may differ by at most 1e-9 relative (a
 * different major-axis baseline is a different depth scale):
 * SVA_ERR_INVALID_ARG otherwise.  lr_check: SVA_ERR_UNSUPPORTED (a frame with
 * several reference cameras has sva_array_depth_checked instead).  Each context
 * that runs a group grows its cost workspace as sva_disparity_sgm_multi_d
 * says.  Synchronous. */
int sva_array_depth_mb(void* multi, const uint8_t* const* images, int n_images, int width,
                       int height, size_t pitch, const sva_array_pair* pairs, int n_pairs,
                       const int32_t* group_start, int n_groups, double f, double pixel_size,
                       int uniqueness, double* depth, uint16_t* maps, uint16_t* cost_min,
                       uint16_t* cost_second);
/* sva_array_depth_mb for groups of UNEQUAL baselines: group g
 * runs one sva_disparity_sgm_mixed_d.  unit_baseline: host [n_groups] f64, > 0;
 * a pair's baseline / unit_baseline[g] must lie within 1e-9 relative of some
 * num/den with both in 1..8 (the smallest den is taken), and its match
 * distance must fit 16 bits: SVA_ERR_INVALID_ARG otherwise.  A group's
 * disparity counts pixels of the unit baseline: depth = unit_baseline[g] * f /
 * ((double)d * pixel_size).  Everything else as sva_array_depth_mb, which keeps
 * refusing such groups. */
int sva_array_depth_mixed(void* multi, const uint8_t* const* images, int n_images, int width,
                          int height, size_t pitch, const sva_array_pair* pairs, int n_pairs,
                          const int32_t* group_start, int n_groups, const double* unit_baseline,
                          double f, double pixel_size, int uniqueness, double* depth,
                          uint16_t* maps, uint16_t* cost_min, uint16_t* cost_second);
/* Sub-pixel depth from an array frame: one entry for the
 * three routes above.  Every job runs with subpixel = 1, whatever
 * pairs[j].params.subpixel says, its f32 map is gathered with its u16 map, and
 * depth comes from sva_fuse_depth_sub_d / sva_fuse_depth_conf_sub_d, so it is
 * not quantised to whole disparities.  The gather ships 4 more bytes per pixel
 * and job than the entry of the same route above.
 *   SVA_ARRAY_PAIRS         as sva_array_depth_conf: mode is SVA_FUSE_MEDIAN,
 *                           _MIN_COST or _MAX_MARGIN, per-pair lr_check works.
 *   SVA_ARRAY_GROUPS        as sva_array_depth_mb.
 *   SVA_ARRAY_GROUPS_MIXED  as sva_array_depth_mixed.
 * On the group routes mode must be SVA_FUSE_MEDIAN and n_valid and winner NULL
 * (one map per group); unit_baseline must be non-NULL for GROUPS_MIXED and NULL
 * for the other routes.  A break of these rules or an unknown route returns
 * SVA_ERR_INVALID_ARG before group_start is read.  subpix (nullable): host
 * [n_jobs][H][W] f32, the jobs' sub-pixel maps (n_jobs = n_pairs, or n_groups
 * on the group routes), NaN where the pixel was rejected.  depth, n_valid,
 * winner, maps, cost_min, cost_second: as for the entry of the same route. */
#define SVA_ARRAY_PAIRS 0
#define SVA_ARRAY_GROUPS 1        /* sva_array_depth_mb's route    */
#define SVA_ARRAY_GROUPS_MIXED 2  /* sva_array_depth_mixed's route */
int sva_array_depth_sub(void* multi, const uint8_t* const* images, int n_images, int width,
                        int height, size_t pitch, const sva_array_pair* pairs, int n_pairs,
                        const int32_t* group_start, int n_groups, int route,
                        const double* unit_baseline, double f, double pixel_size, int uniqueness,
                        int mode, double* depth, uint8_t* n_valid, uint8_t* winner, float* subpix,
                        uint16_t* maps, uint16_t* cost_min, uint16_t* cost_second);
/* An array frame of several reference cameras with the cross-view check
 * (DESIGN.md §2.5b, §7): sva_array_depth_sub's arguments on a GROUP route (so
 * mode is SVA_FUSE_MEDIAN and n_valid and winner are NULL), then the check's;
 * between the gather and the depth step devices[0] runs sva_cross_check_d over
 * the groups' maps, view g being camera pairs[group_start[g]].ref.  maps,
 * subpix and depth are those of the CHECKED maps (depth from sva_fuse_depth_d,
 * or with sub = 1 from sva_fuse_depth_sub_d); cost_min / cost_second are the
 * matcher's.  view_step: host [n_images][2] i32, every camera's position in
 * unit baselines (see sva_cross_check).  sub: 0 = integer depth as
 * sva_array_depth_mb / _mixed (subpix must be NULL), 1 = as sva_array_depth_sub.
 * agree, conflict (nullable): host [n_groups][H][W] u8.  min_agree = 0 with
 * max_conflict = 31 gives the unchecked entry's outputs bit for bit.
 * SVA_ARRAY_PAIRS: SVA_ERR_UNSUPPORTED (its maps share one reference camera:
 * nothing to cross).  sub outside 0 / 1: SVA_ERR_INVALID_ARG, answered first.
 * Then the rules of the route's own entry, and after them, in this order:
 * null view_step; n_groups > 32 (SVA_ERR_UNSUPPORTED); two groups with one ref;
 * groups whose params.invalid differ; groups whose depth scale (the pairs'
 * baseline, or unit_baseline[g] on GROUPS_MIXED) differs by more than 1e-9
 * relative; a pair whose step contradicts view_step -- with M = max(|dir|,
 * |dir_y|), its ratio num/den (1/1 on GROUPS) and e = view_step[other] -
 * view_step[ref], e * M * den must equal (dir, dir_y) * num; then the ranges of
 * sva_cross_check on the groups' view_step, max_diff, min_agree, max_conflict.
 * SVA_ERR_INVALID_ARG unless noted, before anything is launched. */
int sva_array_depth_checked(void* multi, const uint8_t* const* images, int n_images, int width,
                            int height, size_t pitch, const sva_array_pair* pairs, int n_pairs,
                            const int32_t* group_start, int n_groups, int route,
                            const double* unit_baseline, double f, double pixel_size,
                            int uniqueness, int mode, double* depth, uint8_t* n_valid,
                            uint8_t* winner, float* subpix, uint16_t* maps, uint16_t* cost_min,
                            uint16_t* cost_second, const int32_t* view_step, int sub, int max_diff,
                            int min_agree, int max_conflict, uint8_t* agree, uint8_t* conflict);
/* An array frame with the speckle filter:
 * sva_array_depth_checked's arguments, then check, the filter's max_size and
 * max_diff (see sva_filter_speckles) and comp_size (nullable): host
 * [n_jobs][H][W] u32, one plane per map (per pair on SVA_ARRAY_PAIRS, per group
 * on the group routes).  devices[0] runs sva_filter_speckles_d in place over
 * every job's map after the optional cross-view check and before the depth step.
 * check = 1: sva_array_depth_checked plus the filter (group routes only).
 * check = 0: no cross-view check; view_step, max_diff, min_agree, max_conflict
 * are ignored, agree and conflict must be NULL, and every route is accepted: on
 * SVA_ARRAY_PAIRS every pair's map is filtered before its group's fusion, with
 * every mode and with per-pair lr_check.  maps, subpix, depth, n_valid and
 * winner are those of the FILTERED maps; cost_min / cost_second are the
 * matcher's.  Bit for bit: speckle_max_size = 0 gives sva_array_depth_checked's
 * outputs (check = 1), sva_array_depth_sub's (check = 0, sub = 1) or those of
 * the route's own entry -- sva_array_depth_conf, _mb, _mixed -- (check = 0, sub
 * = 0); any other value gives the stand-alone composition: the unfiltered
 * frame's maps through sva_cross_check (check = 1), sva_filter_speckles and the
 * matching sva_fuse_depth*.
 * sub outside 0 / 1: SVA_ERR_INVALID_ARG, answered first.  Then the rules of
 * sva_array_depth_checked (check = 1) or of the route's own entry and of
 * sva_array_depth_sub's shared argument list (check = 0), and after them, in
 * this order, SVA_ERR_INVALID_ARG for: check outside 0 / 1; with check = 0, a
 * non-NULL agree or conflict, then a subpix plane with sub = 0;
 * speckle_max_size < 0; speckle_max_diff < 0.  Before anything is launched. */
int sva_array_depth_filtered(void* multi, const uint8_t* const* images, int n_images, int width,
                             int height, size_t pitch, const sva_array_pair* pairs, int n_pairs,
                             const int32_t* group_start, int n_groups, int route,
                             const double* unit_baseline, double f, double pixel_size,
                             int uniqueness, int mode, double* depth, uint8_t* n_valid,
                             uint8_t* winner, float* subpix, uint16_t* maps, uint16_t* cost_min,
                             uint16_t* cost_second, const int32_t* view_step, int sub,
                             int max_diff, int min_agree, int max_conflict, uint8_t* agree,
                             uint8_t* conflict, int check, int speckle_max_size,
                             int speckle_max_diff, uint32_t* comp_size);
/* An array frame with hole filling:
 * sva_array_depth_filtered's arguments, then the fill's max_dist, min_found and
 * mode (see sva_fill_holes) and n_found (nullable): host [n_jobs][H][W] u8, one
 * plane per map (per pair on SVA_ARRAY_PAIRS, per group on the group routes).
 * devices[0] runs sva_fill_holes_d in place over every job's map -- and its f32
 * plane with sub = 1 -- after the speckle filter and before the depth step, on
 * every route; on SVA_ARRAY_PAIRS per pair, before the group's fusion.  maps,
 * subpix, depth, n_valid and winner are those of the FILLED maps; cost_min /
 * cost_second stay the matcher's: at a filled pixel they describe the match
 * that was rejected, not the value filled in, so SVA_FUSE_MEDIAN is the sensible
 * fusion mode after a fill.  Bit for bit: fill_max_dist = 0 gives
 * sva_array_depth_filtered's outputs; any other value gives the stand-alone
 * composition: the filtered frame's maps through sva_fill_holes and the
 * matching sva_fuse_depth*.
 * After all of sva_array_depth_filtered's rules, in this order,
 * SVA_ERR_INVALID_ARG for: fill_max_dist outside 0..255; fill_min_found outside
 * 1..8; fill_mode outside 0..2.  Before anything is launched. */
int sva_array_depth_filled(void* multi, const uint8_t* const* images, int n_images, int width,
                           int height, size_t pitch, const sva_array_pair* pairs, int n_pairs,
                           const int32_t* group_start, int n_groups, int route,
                           const double* unit_baseline, double f, double pixel_size,
                           int uniqueness, int mode, double* depth, uint8_t* n_valid,
                           uint8_t* winner, float* subpix, uint16_t* maps, uint16_t* cost_min,
                           uint16_t* cost_second, const int32_t* view_step, int sub, int max_diff,
                           int min_agree, int max_conflict, uint8_t* agree, uint8_t* conflict,
                           int check, int speckle_max_size, int speckle_max_diff,
                           uint32_t* comp_size, int fill_max_dist, int fill_min_found,
                           int fill_mode, uint8_t* n_found);
/* An array frame with the weighted median filter:
 * sva_array_depth_filled's arguments, then wmed_radius, wmed_weights (a host
 * array of 256 u16; null: the unguided filter), wmed_min_support, wmed_select
 * and support (nullable): host [n_jobs][H][W] u16, one plane per map.
 * devices[0] runs sva_weighted_median_d with fill = 1 over every job's map --
 * and its f32 plane with sub = 1 -- after the fill and before the depth step, on
 * every route; the guide of a job is its reference view, which is uploaded to
 * devices[0] as well if the job ran elsewhere.  wmed_select = 0 filters every
 * pixel; 1 filters only the pixels the fill looked at: the fill's n_found plane
 * is the select plane (kept even if n_found is null), so with fill_max_dist = 0
 * it changes nothing and the outputs are sva_array_depth_filled's bit for bit.
 * maps, subpix, depth, n_valid and winner are those of the SMOOTHED maps; the
 * cost planes stay the matcher's, so SVA_FUSE_MEDIAN is the sensible fusion mode.
 * Bit for bit the stand-alone composition: the filled frame's maps through
 * sva_weighted_median and the matching sva_fuse_depth*.
 * After all of sva_array_depth_filled's rules, in this order,
 * SVA_ERR_INVALID_ARG for: wmed_radius outside 1..15; wmed_min_support outside
 * 1..961; wmed_select outside 0..1.  Before anything is launched. */
int sva_array_depth_smoothed(void* multi, const uint8_t* const* images, int n_images, int width,
                             int height, size_t pitch, const sva_array_pair* pairs, int n_pairs,
                             const int32_t* group_start, int n_groups, int route,
                             const double* unit_baseline, double f, double pixel_size,
                             int uniqueness, int mode, double* depth, uint8_t* n_valid,
                             uint8_t* winner, float* subpix, uint16_t* maps, uint16_t* cost_min,
                             uint16_t* cost_second, const int32_t* view_step, int sub,
                             int max_diff, int min_agree, int max_conflict, uint8_t* agree,
                             uint8_t* conflict, int check, int speckle_max_size,
                             int speckle_max_diff, uint32_t* comp_size, int fill_max_dist,
                             int fill_min_found, int fill_mode, uint8_t* n_found, int wmed_radius,
                             const uint16_t* wmed_weights, int wmed_min_support, int wmed_select,
                             uint16_t* support);
/* An array frame from RAW views: sva_array_depth_smoothed's
 * arguments, then rect (a host array of n_images sva_rectify_view), border, mask
 * (0 / 1), views_out and valid_out (nullable host [n_images][H][W] u8).  images
 * are the raw views, of the frame's size.  Every device rectifies the views it
 * needs with one sva_rectify_d launch on its copy stream, behind their uploads,
 * and the jobs wait for that launch; everything after it sees rectified views.
 * With mask = 1 every job's map -- and its f32 plane with sub = 1 -- goes through
 * sva_mask_maps_d with the valid plane of its reference view, after the gather
 * and before the cross-view check, on every route (on SVA_ARRAY_PAIRS per pair).
 * views_out / valid_out receive the rectified views and their valid planes; a
 * view that no pair names is left untouched.  Every stage of the chain can be
 * switched off here: wmed_radius = 0 turns the weighted median off for this
 * entry only (the outputs are then sva_array_depth_filled's bit for bit, support
 * is left untouched), the other stages have their own off value.
 * Bit for bit the stand-alone composition: sva_rectify; the same route's plain
 * job maps on the rectified views; sva_mask_maps, sva_cross_check,
 * sva_filter_speckles, sva_fill_holes, sva_weighted_median; the matching
 * sva_fuse_depth*.
 * After all of sva_array_depth_smoothed's rules (wmed_radius 0 allowed), in this
 * order, SVA_ERR_INVALID_ARG for: a null rect; the first rule a view of rect
 * breaks (sva_rectify's, view 0 first); border outside 0..255; mask outside
 * 0..1.  Before anything is launched. */
int sva_array_depth_rectified(void* multi, const uint8_t* const* images, int n_images, int width,
                              int height, size_t pitch, const sva_array_pair* pairs, int n_pairs,
                              const int32_t* group_start, int n_groups, int route,
                              const double* unit_baseline, double f, double pixel_size,
                              int uniqueness, int mode, double* depth, uint8_t* n_valid,
                              uint8_t* winner, float* subpix, uint16_t* maps, uint16_t* cost_min,
                              uint16_t* cost_second, const int32_t* view_step, int sub,
                              int max_diff, int min_agree, int max_conflict, uint8_t* agree,
                              uint8_t* conflict, int check, int speckle_max_size,
                              int speckle_max_diff, uint32_t* comp_size, int fill_max_dist,
                              int fill_min_found, int fill_mode, uint8_t* n_found, int wmed_radius,
                              const uint16_t* wmed_weights, int wmed_min_support, int wmed_select,
                              uint16_t* support, const sva_rectify_view* rect, int border,
                              int mask, uint8_t* views_out, uint8_t* valid_out);

#ifdef __cplusplus
}
#endif
#endif /* SVA_H */
