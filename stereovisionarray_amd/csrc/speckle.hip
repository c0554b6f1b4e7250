// speckle.hip -- the speckle filter: connected components of the disparity maps
// and the removal of the small ones.
//
// Four launches on the context stream over two u32 planes [n][H][W] of
// workspace, `label` and `count`; the only ordering between them is the launch
// boundary (speckle_uf.h has the union-find and its invariants):
//   speckle_label  one workgroup per tile of one map: the tile's inner links by
//                  union-find in LDS; label[p] = the in-map index of p's
//                  tile-local root (the smallest index of its component within
//                  the tile; kNoLabel where p is not valid), count[p] = the
//                  tile-local component's size at that root, 0 elsewhere.
//   speckle_merge  one thread per link across a tile border: unite on the global
//                  labels.  Every access to the label plane is an agent-scope
//                  relaxed atomic; the algorithm is right for any earlier value
//                  a load may return.
//   speckle_count  every tile-local root p whose global root r differs adds its
//                  count to count[r] (one global atomic per tile-local
//                  component, not per pixel) and points label[p] at r.
//   speckle_apply  r = find(p), size = count[r]: out, out_sub, comp_size.
// Every access is of the element's own size (a u16 plane at odd W has 2-byte
// aligned rows, and so may its base).  In-map indices are u32 (W * H < 2^31),
// plane offsets size_t.  out may be disps and out_sub subpix: the apply pass
// reads and writes a pixel in one thread, and the earlier passes only read.
#include "speckle_math.h"
#include "speckle_uf.h"
#include "sva_internal.h"

namespace sva {
namespace {

constexpr int TW = tune::kSpeckleTileW, TH = tune::kSpeckleTileH, TP = TW * TH;
constexpr int kThreads = 256;
constexpr int kPer = TP / kThreads;        // pixels of a tile per thread
static_assert(TP % kThreads == 0 && kPer >= 1, "a tile is a whole number of passes");
constexpr unsigned kMaxGridY = 65535;      // maps beyond this are walked by stride

// The tile's labels in LDS: workgroup-scope relaxed atomics.
struct LdsLabels {
    uint32_t* l;
    __device__ uint32_t load(uint32_t i) {
        return __hip_atomic_load(&l[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __device__ uint32_t min_exchange(uint32_t i, uint32_t v) {
        return __hip_atomic_fetch_min(&l[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};

// One map's label plane while other workgroups modify it: agent-scope relaxed atomics.
struct GlobalLabels {
    uint32_t* l;
    __device__ uint32_t load(uint32_t i) {
        return __hip_atomic_load(&l[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ uint32_t min_exchange(uint32_t i, uint32_t v) {
        return __hip_atomic_fetch_min(&l[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// A label plane that nothing modifies in this launch.
struct FrozenLabels {
    const uint32_t* l;
    __device__ uint32_t load(uint32_t i) { return l[i]; }
};

__global__ __launch_bounds__(kThreads) void speckle_label_kernel(
    const uint16_t* __restrict__ disps, int n, int W, int H, unsigned np, unsigned tiles_x,
    unsigned invalid, int max_diff, uint32_t* __restrict__ label, uint32_t* __restrict__ count) {
    __shared__ uint16_t sd[TP];
    __shared__ uint32_t sl[TP];
    __shared__ uint32_t sc[TP];
    const int x0 = (int)(blockIdx.x % tiles_x) * TW, y0 = (int)(blockIdx.x / tiles_x) * TH;
    LdsLabels lds{sl};
    for (unsigned m = blockIdx.y; m < (unsigned)n; m += gridDim.y) {
        const size_t base = (size_t)m * np;
        for (int i = threadIdx.x; i < TP; i += kThreads) {
            const int x = x0 + i % TW, y = y0 + i / TW;
            // a pixel outside the frame is 0: not valid, linked to nothing
            sd[i] = x < W && y < H ? disps[base + (size_t)y * W + x] : (uint16_t)0;
            sl[i] = (uint32_t)i;
            sc[i] = 0u;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < TP; i += kThreads) {
            const unsigned s = sd[i];
            if (i % TW + 1 < TW && sp::linked(s, sd[i + 1], invalid, max_diff))
                uf::unite(lds, (uint32_t)i, (uint32_t)i + 1);
            if (i / TW + 1 < TH && sp::linked(s, sd[i + TW], invalid, max_diff))
                uf::unite(lds, (uint32_t)i, (uint32_t)i + TW);
        }
        __syncthreads();
        uint32_t root[kPer];
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            const int i = threadIdx.x + k * kThreads;
            root[k] = sp::kNoLabel;
            if (cc::valid(sd[i], invalid)) {
                root[k] = uf::find(lds, (uint32_t)i);
                atomicAdd(&sc[root[k]], 1u);
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            const int i = threadIdx.x + k * kThreads;
            const int x = x0 + i % TW, y = y0 + i / TW;
            if (x < W && y < H) {
                const uint32_t r = root[k];
                const size_t at = base + (size_t)y * W + x;
                // the local root's in-map index: the order of tile indices is
                // the order of in-map indices, so it is the smallest of both
                label[at] = r == sp::kNoLabel
                                ? sp::kNoLabel
                                : (uint32_t)(y0 + (int)(r / TW)) * (uint32_t)W + (uint32_t)(x0 + (int)(r % TW));
                count[at] = r == (uint32_t)i ? sc[i] : 0u;
            }
        }
        __syncthreads();   // the next map reuses the LDS planes
    }
}

// Links across tile borders, per map: (tiles_x - 1) * H between columns
// k * TW - 1 and k * TW, then (tiles_y - 1) * W between rows k * TH - 1 and k * TH.
__global__ __launch_bounds__(kThreads) void speckle_merge_kernel(
    const uint16_t* __restrict__ disps, int n, int W, int H, unsigned np, unsigned tiles_x,
    unsigned tiles_y, unsigned invalid, int max_diff, uint32_t* label) {
    const unsigned vx = tiles_x - 1, n_vert = vx * (unsigned)H;
    const unsigned n_edges = n_vert + (tiles_y - 1) * (unsigned)W;
    const unsigned e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= n_edges) return;
    uint32_t a, b;
    if (e < n_vert) {
        const unsigned y = e / vx, x = (e % vx + 1) * TW;   // x <= (tiles_x - 1) * TW < W
        a = y * (unsigned)W + x - 1;
        b = a + 1;
    } else {
        const unsigned f = e - n_vert;
        const unsigned y = (f / (unsigned)W + 1) * TH, x = f % (unsigned)W;   // y < H likewise
        b = y * (unsigned)W + x;
        a = b - (unsigned)W;
    }
    for (unsigned m = blockIdx.y; m < (unsigned)n; m += gridDim.y) {
        const size_t base = (size_t)m * np;
        if (!sp::linked(disps[base + a], disps[base + b], invalid, max_diff)) continue;
        GlobalLabels g{label + base};
        uf::unite(g, a, b);
    }
}

__global__ __launch_bounds__(kThreads) void speckle_count_kernel(int n, unsigned np,
                                                                 uint32_t* label, uint32_t* count) {
    const unsigned p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= np) return;
    for (unsigned m = blockIdx.y; m < (unsigned)n; m += gridDim.y) {
        const size_t base = (size_t)m * np;
        // count[p] > 0 only at a tile-local root; the adds below go to global
        // roots, which are tile-local roots too, so the test reads > 0 either way
        const uint32_t c = __hip_atomic_load(&count[base + p], __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        if (c == 0u) continue;
        GlobalLabels g{label + base};
        const uint32_t r = uf::find(g, p);
        if (r == p) continue;
        // p is not a global root: nothing is ever added to count[p], so c is its tile's count
        atomicAdd(&count[base + r], c);
        g.min_exchange(p, r);   // path compression: labels only decrease
    }
}

// label null: max_size = 0 with no comp_size, a copy.
__global__ __launch_bounds__(kThreads) void speckle_apply_kernel(
    const uint16_t* disps, const float* subpix, int n, unsigned np, unsigned invalid, int max_size,
    const uint32_t* __restrict__ label, const uint32_t* __restrict__ count, uint16_t* out,
    float* out_sub, uint32_t* __restrict__ comp_size) {
    const unsigned p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= np) return;
    for (unsigned m = blockIdx.y; m < (unsigned)n; m += gridDim.y) {
        const size_t base = (size_t)m * np, at = base + p;
        const unsigned s = disps[at];
        uint32_t size = 0u;
        if (label && cc::valid(s, invalid)) {
            FrozenLabels g{label + base};
            size = count[base + uf::find(g, p)];
        }
        const bool gone = sp::removed(size, max_size);
        out[at] = (uint16_t)(gone ? invalid : s);
        if (out_sub) out_sub[at] = gone ? __builtin_nanf("") : subpix[at];
        if (comp_size) comp_size[at] = size;
    }
}

}  // namespace

hipError_t launch_speckle(Ctx& c, const uint16_t* disps, const float* subpix, int n, int W, int H,
                          uint16_t invalid, int max_size, int max_diff, uint32_t* label,
                          uint32_t* count, uint16_t* out, float* out_sub, uint32_t* comp_size) {
    const unsigned long long np64 = (unsigned long long)W * (unsigned long long)H;
    if (n < 1 || W <= 0 || H <= 0 || np64 >= (1ull << 31) || max_size < 0 || max_diff < 0 ||
        (out_sub && !subpix) || !disps || !out || (label == nullptr) != (count == nullptr) ||
        (!label && (max_size != 0 || comp_size)))
        return hipErrorInvalidValue;
    const unsigned np = (unsigned)np64;
    const unsigned tiles_x = ((unsigned)W + TW - 1) / TW, tiles_y = ((unsigned)H + TH - 1) / TH;
    const unsigned gy = (unsigned)n < kMaxGridY ? (unsigned)n : kMaxGridY;
    const unsigned pix_blocks = (np + kThreads - 1) / kThreads;
    const int md = sp::clamp_diff(max_diff);
    hipError_t e = hipSuccess;
    if (label) {
        {
            ScopedKernelTimer t(c, "speckle_label");
            hipLaunchKernelGGL(speckle_label_kernel, dim3(tiles_x * tiles_y, gy), dim3(kThreads), 0,
                               c.stream, disps, n, W, H, np, tiles_x, (unsigned)invalid, md, label,
                               count);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        {
            // fewer than 2 * W * H / min(TW, TH) links; a frame of one tile has none
            const unsigned edges = (tiles_x - 1) * (unsigned)H + (tiles_y - 1) * (unsigned)W;
            const unsigned blocks = edges ? (edges + kThreads - 1) / kThreads : 1u;
            ScopedKernelTimer t(c, "speckle_merge");
            hipLaunchKernelGGL(speckle_merge_kernel, dim3(blocks, gy), dim3(kThreads), 0, c.stream,
                               disps, n, W, H, np, tiles_x, tiles_y, (unsigned)invalid, md, label);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        {
            ScopedKernelTimer t(c, "speckle_count");
            hipLaunchKernelGGL(speckle_count_kernel, dim3(pix_blocks, gy), dim3(kThreads), 0,
                               c.stream, n, np, label, count);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
    }
    ScopedKernelTimer t(c, "speckle_apply");
    hipLaunchKernelGGL(speckle_apply_kernel, dim3(pix_blocks, gy), dim3(kThreads), 0, c.stream,
                       disps, subpix, n, np, (unsigned)invalid, max_size, (const uint32_t*)label,
                       (const uint32_t*)count, out, out_sub, comp_size);
    return hipGetLastError();
}

}  // namespace sva
