// wmedian.hip -- the weighted median filter: every considered pixel of the
// disparity maps takes the lower weighted median of its window's valid pixels,
// weighted by how close the guide image is to the centre's intensity (DESIGN.md
// §2.5e, §4.24).
//
// One launch on the context stream.  A workgroup of kWmedTileW x kWmedTileH
// threads owns one output tile at a time (tiles and maps by stride).  Per tile:
//   1. every thread reads its own d, select and decides `considered`; a tile
//      without a considered pixel copies and goes on -- nothing is staged;
//   2. the tile plus an r-wide halo is staged in LDS, d as wm::staged (0 for a
//      hole or a cell outside the frame: "not a candidate") and, guided, g; the
//      256-entry table is staged once per workgroup;
//   3. a considered thread runs wm::pick over its window (wmedian_math.h): the
//      inner loops read LDS only and test no bound.
// Every global access is of the element's own size (a u16 plane at odd W has
// 2-byte aligned rows, and so may its base; a guide may start at any byte).
// In-map indices are u32 (W * H < 2^31), plane and guide offsets size_t.  The
// outputs overlap no input (sva_api.cpp refuses it): other workgroups read the
// cells this one writes.
#include "sva_internal.h"
#include "sva_tuning.h"
#include "wmedian_math.h"

namespace sva {
namespace {

constexpr int kTW = tune::kWmedTileW, kTH = tune::kWmedTileH;
constexpr int kThreads = kTW * kTH;
constexpr int kCells = (kTW + 2 * wm::kMaxRadius) * (kTH + 2 * wm::kMaxRadius);
static_assert(kThreads >= wm::kWeights && kThreads <= 1024, "one thread per table entry");
constexpr unsigned kMaxGridX = 1u << 20;   // tiles beyond this are walked by stride
constexpr unsigned kMaxGridY = 65535;      // and so are maps

// The kernel's arguments, by value: the table and the guides of one launch
// travel in the kernel-argument segment, so the host arrays are read before
// the launch call returns and no device copy of them has to be kept alive.
struct WmedArgs {
    const uint16_t* disps;
    const float* subpix;
    const uint8_t* select;
    uint16_t* out;
    float* out_sub;
    uint16_t* support;
    size_t gpitch;
    unsigned np;
    int n, W, H, r, min_support, fill;
    unsigned invalid;
    uint16_t w[wm::kWeights];
    const uint8_t* g[tune::kWmedLaunchMaps];
};

struct Window {
    const uint16_t* d0;   // the window's top-left cell
    const uint8_t* g0;
    const uint16_t* tab;
    int stride;
    __device__ unsigned d(int i, int j) const { return d0[j * stride + i]; }
    __device__ unsigned g(int i, int j) const { return g0[j * stride + i]; }
    __device__ unsigned w(int delta) const { return tab[delta]; }
};

template <bool GUIDED>
__global__ __launch_bounds__(kThreads) void wmedian_kernel(const WmedArgs a) {
    __shared__ uint16_t sd[kCells];
    __shared__ uint8_t sg[GUIDED ? kCells : 1];
    __shared__ uint16_t tab[GUIDED ? wm::kWeights : 1];
    const int tx = (int)threadIdx.x, ty = (int)threadIdx.y;
    const int r = a.r, W = a.W, H = a.H;
    const int sw = kTW + 2 * r, sh = kTH + 2 * r;
    if (GUIDED) {
        const int t = ty * kTW + tx;
        if (t < wm::kWeights) tab[t] = a.w[t];
    }
    const unsigned tiles_x = ((unsigned)W + kTW - 1) / kTW, tiles_y = ((unsigned)H + kTH - 1) / kTH;
    const unsigned tiles = tiles_x * tiles_y;   // <= W * H < 2^31
    for (unsigned m = blockIdx.y; m < (unsigned)a.n; m += gridDim.y) {
        const size_t base = (size_t)m * a.np;
        const uint16_t* dm = a.disps + base;
        const uint8_t* gm = GUIDED ? a.g[m] : nullptr;
        for (unsigned t = blockIdx.x; t < tiles; t += gridDim.x) {
            const int x0 = (int)(t % tiles_x) * kTW, y0 = (int)(t / tiles_x) * kTH;
            const int x = x0 + tx, y = y0 + ty;
            const bool in = x < W && y < H;
            const unsigned p = in ? (unsigned)y * (unsigned)W + (unsigned)x : 0u;
            const unsigned own = in ? dm[p] : 0u;
            const unsigned sel = !in ? 0u : a.select ? a.select[base + p] : 1u;
            const bool look = wm::considered(sel, a.fill, own, a.invalid);
            // a barrier too: the last tile's windows are read before this one is staged
            const bool any = __syncthreads_or(look) != 0;
            if (any) {
                for (int cy = ty; cy < sh; cy += kTH)
                    for (int cx = tx; cx < sw; cx += kTW) {
                        const int qx = x0 - r + cx, qy = y0 - r + cy;
                        const bool q_in = qx >= 0 && qx < W && qy >= 0 && qy < H;
                        unsigned v = 0;
                        if (q_in) v = wm::staged(dm[(unsigned)qy * (unsigned)W + (unsigned)qx], a.invalid);
                        sd[cy * sw + cx] = (uint16_t)v;
                        if (GUIDED) sg[cy * sw + cx] = q_in ? gm[(size_t)qy * a.gpitch + (size_t)qx] : 0;
                    }
                __syncthreads();
            }
            if (!in) continue;
            unsigned v = own, n = 0;
            size_t src = base + p;
            if (look) {
                const Window win{sd + ty * sw + tx, GUIDED ? sg + ty * sw + tx : nullptr, tab, sw};
                const int gp = GUIDED ? (int)sg[(ty + r) * sw + tx + r] : 0;
                const wm::Pick k = wm::pick<GUIDED>(win, r, gp, a.min_support);
                n = k.n;
                if (k.written) {
                    v = k.d;
                    // the source is a valid pixel of the frame: it was staged as one
                    src = base + (size_t)(y + k.j - r) * (size_t)W + (size_t)(x + k.i - r);
                }
            }
            a.out[base + p] = (uint16_t)v;
            if (a.out_sub) a.out_sub[base + p] = a.subpix[src];
            if (a.support) a.support[base + p] = (uint16_t)n;
        }
    }
}

}  // namespace

hipError_t launch_wmedian(Ctx& c, const uint16_t* disps, const float* subpix,
                          const uint8_t* const* guides, size_t guide_pitch, const uint16_t* weights,
                          const uint8_t* select, int n, int W, int H, uint16_t invalid, int radius,
                          int min_support, int fill, uint16_t* out, float* out_sub,
                          uint16_t* support) {
    const unsigned long long np64 = (unsigned long long)W * (unsigned long long)H;
    if (n < 1 || W <= 0 || H <= 0 || np64 >= (1ull << 31) || !disps || !out ||
        wm::thresholds_error(radius, min_support, fill) || (out_sub && !subpix) ||
        (guides == nullptr) != (weights == nullptr) || (guides && guide_pitch < (size_t)W))
        return hipErrorInvalidValue;
    const unsigned np = (unsigned)np64;
    const unsigned tiles = ((unsigned)W + kTW - 1) / kTW * (((unsigned)H + kTH - 1) / kTH);
    ScopedKernelTimer t(c, "wmed");
    for (int m0 = 0; m0 < n; m0 += tune::kWmedLaunchMaps) {
        const int nm = n - m0 < tune::kWmedLaunchMaps ? n - m0 : tune::kWmedLaunchMaps;
        const size_t at = (size_t)m0 * np;
        WmedArgs a{};
        a.disps = disps + at;
        a.subpix = subpix ? subpix + at : nullptr;
        a.select = select ? select + at : nullptr;
        a.out = out + at;
        a.out_sub = out_sub ? out_sub + at : nullptr;
        a.support = support ? support + at : nullptr;
        a.gpitch = guide_pitch;
        a.np = np;
        a.n = nm;
        a.W = W;
        a.H = H;
        a.r = radius;
        a.min_support = min_support;
        a.fill = fill;
        a.invalid = invalid;
        if (guides) {
            for (int i = 0; i < wm::kWeights; i++) a.w[i] = weights[i];
            for (int i = 0; i < nm; i++) {
                if (!guides[m0 + i]) return hipErrorInvalidValue;
                a.g[i] = guides[m0 + i];
            }
        }
        const dim3 grid(tiles < kMaxGridX ? tiles : kMaxGridX,
                        (unsigned)nm < kMaxGridY ? (unsigned)nm : kMaxGridY);
        if (guides)
            hipLaunchKernelGGL(wmedian_kernel<true>, grid, dim3(kTW, kTH), 0, c.stream, a);
        else
            hipLaunchKernelGGL(wmedian_kernel<false>, grid, dim3(kTW, kTH), 0, c.stream, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace sva
