// rectify.hip -- rectification: n raw views warped onto the ideal grid by a
// homography and a Brown-Conrady model per view, and
// sva_mask_maps (§2.5g), which takes a view's valid plane to its disparity map.
//
// rectify_kernel: one launch for up to kRectLaunchViews views, the view in
// grid.z, its sva_rectify_view in the kernel-argument segment (read with scalar
// loads; no device copy of the host table has to be kept alive).  A thread owns
// kRectPixels = 4 horizontally adjacent output pixels: it runs rc::sample
// (rectify_math.h: the f64 chain, not contracted; four byte gathers through the
// cache) once per pixel and stores the four bytes as one dword.  The groups of
// four start where the output ROW's address is a multiple of 4, not at x = 0,
// so the dword store is aligned at every base and pitch; the pixels of a group
// that straddles x = 0 or x = W are stored as bytes.  valid follows out's groups
// and takes the dword store where its own address allows it; map is written as
// dwords.  Both are skipped by a uniform branch when null.
//
// mask_kernel: one thread per pixel, by stride.
#include "rectify_math.h"
#include "sva_internal.h"
#include "sva_tuning.h"

#pragma clang fp contract(off)

namespace sva {
namespace {

constexpr int kPix = tune::kRectPixels;
constexpr int kBX = tune::kRectBlockX, kBY = tune::kRectBlockY;
static_assert(kPix == 4, "a group of pixels is one dword");

struct RectArgs {
    const uint8_t* src;
    uint8_t* out;
    uint8_t* valid;
    int32_t* map;
    size_t src_pitch, out_pitch;
    int sw, sh, W, H;
    unsigned border;
    sva_rectify_view v[tune::kRectLaunchViews];
};
static_assert(sizeof(RectArgs) <= 4096, "the kernel-argument segment");

struct SrcTap {
    const uint8_t* base;
    size_t pitch;
    __device__ unsigned operator()(int X, int Y) const {
        return base[(size_t)Y * pitch + (size_t)X];
    }
};

__global__ __launch_bounds__(kBX * kBY) void rectify_kernel(const RectArgs a) {
    const int view = (int)blockIdx.z;
    const int y = (int)(blockIdx.y * kBY + threadIdx.y);
    if (y >= a.H) return;
    const size_t row = ((size_t)view * (size_t)a.H + (size_t)y) * a.out_pitch;
    uint8_t* orow = a.out + row;
    const int mis = (int)((uintptr_t)orow & 3u);
    const int x0 = (int)(blockIdx.x * kBX + threadIdx.x) * kPix - mis;
    if (x0 >= a.W) return;
    const sva_rectify_view& v = a.v[view];
    const bool distort = rc::has_distortion(v);
    const SrcTap tap{a.src + (size_t)view * (size_t)a.sh * a.src_pitch, a.src_pitch};
    unsigned val = 0, ok = 0;
    int32_t q[2 * kPix];
#pragma unroll
    for (int i = 0; i < kPix; i++) {
        const int x = x0 + i;
        rc::Sample s{rc::kOutside, rc::kOutside, 0u, 0u};
        if (x >= 0 && x < a.W) s = rc::sample(v, distort, x, y, a.sw, a.sh, a.border, tap);
        val |= s.value << (8 * i);
        ok |= s.valid << (8 * i);
        q[2 * i] = s.qx;
        q[2 * i + 1] = s.qy;
    }
    const bool whole = x0 >= 0 && x0 + kPix <= a.W;   // then orow + x0 is 4-aligned
    if (whole) {
        *(uint32_t*)(orow + x0) = val;
    } else {
        for (int i = 0; i < kPix; i++)
            if (x0 + i >= 0 && x0 + i < a.W) orow[x0 + i] = (uint8_t)(val >> (8 * i));
    }
    if (a.valid) {
        uint8_t* vrow = a.valid + row;
        if (whole && (((uintptr_t)(vrow + x0)) & 3u) == 0) {
            *(uint32_t*)(vrow + x0) = ok;
        } else {
            for (int i = 0; i < kPix; i++)
                if (x0 + i >= 0 && x0 + i < a.W) vrow[x0 + i] = (uint8_t)(ok >> (8 * i));
        }
    }
    if (a.map) {
        int32_t* mrow = a.map + ((size_t)view * (size_t)a.H + (size_t)y) * (size_t)a.W * 2;
        for (int i = 0; i < kPix; i++)
            if (x0 + i >= 0 && x0 + i < a.W) {
                mrow[2 * (size_t)(x0 + i)] = q[2 * i];
                mrow[2 * (size_t)(x0 + i) + 1] = q[2 * i + 1];
            }
    }
}

constexpr unsigned kMaskThreads = 256;
constexpr unsigned kMaskMaxBlocks = 1u << 16;

__global__ __launch_bounds__(kMaskThreads) void mask_kernel(
    const uint16_t* disps, const float* subpix, const uint8_t* __restrict__ valid, size_t total,
    unsigned invalid, uint16_t* out, float* out_sub) {
    const size_t stride = (size_t)gridDim.x * kMaskThreads;
    for (size_t p = (size_t)blockIdx.x * kMaskThreads + threadIdx.x; p < total; p += stride) {
        const unsigned ok = valid[p];
        out[p] = (uint16_t)rc::masked(disps[p], ok, invalid);
        if (out_sub) out_sub[p] = ok ? subpix[p] : __builtin_nanf("");
    }
}

}  // namespace

hipError_t launch_rectify(Ctx& c, const uint8_t* src, int n, int sw, int sh, size_t src_pitch,
                          const sva_rectify_view* views, int W, int H, size_t out_pitch,
                          int border, uint8_t* out, uint8_t* valid, int32_t* map) {
    if (!src || !views || !out || n < 1 || sw < 1 || sh < 1 || W < 1 || H < 1 ||
        sw > rc::kMaxSize || sh > rc::kMaxSize || W > rc::kMaxSize || H > rc::kMaxSize ||
        src_pitch < (size_t)sw || out_pitch < (size_t)W || border < 0 || border > 255)
        return hipErrorInvalidValue;
    ScopedKernelTimer t(c, "rectify");
    // + 3: a row's first group may hold one pixel only
    const unsigned groups = ((unsigned)W + 3u + (unsigned)kPix - 1u) / (unsigned)kPix;
    for (int v0 = 0; v0 < n; v0 += tune::kRectLaunchViews) {
        const int nv = n - v0 < tune::kRectLaunchViews ? n - v0 : tune::kRectLaunchViews;
        RectArgs a{};
        a.src = src + (size_t)v0 * (size_t)sh * src_pitch;
        a.out = out + (size_t)v0 * (size_t)H * out_pitch;
        a.valid = valid ? valid + (size_t)v0 * (size_t)H * out_pitch : nullptr;
        a.map = map ? map + (size_t)v0 * (size_t)H * (size_t)W * 2 : nullptr;
        a.src_pitch = src_pitch;
        a.out_pitch = out_pitch;
        a.sw = sw;
        a.sh = sh;
        a.W = W;
        a.H = H;
        a.border = (unsigned)border;
        for (int i = 0; i < nv; i++) a.v[i] = views[v0 + i];
        const dim3 grid((groups + kBX - 1) / kBX, ((unsigned)H + kBY - 1) / kBY, (unsigned)nv);
        hipLaunchKernelGGL(rectify_kernel, grid, dim3(kBX, kBY), 0, c.stream, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_mask_maps(Ctx& c, const uint16_t* disps, const float* subpix,
                            const uint8_t* valid, int n, int W, int H, uint16_t invalid,
                            uint16_t* out, float* out_sub) {
    if (!disps || !valid || !out || n < 1 || W < 1 || H < 1 || (out_sub && !subpix))
        return hipErrorInvalidValue;
    const size_t total = (size_t)W * (size_t)H * (size_t)n;
    const size_t want = (total + kMaskThreads - 1) / kMaskThreads;
    const unsigned blocks = want < kMaskMaxBlocks ? (unsigned)want : kMaskMaxBlocks;
    ScopedKernelTimer t(c, "mask_maps");
    hipLaunchKernelGGL(mask_kernel, dim3(blocks), dim3(kMaskThreads), 0, c.stream, disps, subpix,
                       valid, total, (unsigned)invalid, out, out_sub);
    return hipGetLastError();
}

}  // namespace sva
