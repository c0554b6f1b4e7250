// fill.hip -- hole filling: every hole of the disparity maps takes a low-order
// statistic of the nearest valid pixels along eight directions (DESIGN.md
// §2.5d, §4.23).
//
// Two launches on the context stream over a workspace of eight u32 key planes
// per map, keys [n][8][H][W]; the only ordering between them is the launch
// boundary:
//   fill_scan   one thread per direction, line and segment of kFillSegment steps
//               (fill_math.h scan_segment): it walks the line against the
//               direction, carries the last valid value and the steps since, and
//               writes that direction's key -- or kAbsent -- at EVERY pixel of
//               its segment, so the planes need no memset and the work does not
//               depend on where the holes lie.  The threads of a workgroup are
//               neighbouring lines: for the vertical and diagonal directions
//               (wrapped rows) a step reads and writes one contiguous run.
//   fill_apply  one thread per pixel: a hole sorts its eight keys, picks by
//               mode and writes out, out_sub (gathered from the source pixel
//               p + j * r_k, a valid pixel) and n_found.
// Every access is of the element's own size (a u16 plane at odd W has 2-byte
// aligned rows, and so may its base).  In-map indices are u32 (W * H < 2^31),
// plane offsets size_t.  out may be disps and out_sub subpix: the scan only
// reads; the apply pass reads disps[p] in the thread that writes out[p], reads
// subpix elsewhere only at valid pixels, and in place writes nothing at a pixel
// it does not fill.
#include "fill_math.h"
#include "sva_internal.h"

namespace sva {
namespace {

constexpr int kThreads = 256;
constexpr unsigned kMaxGridZ = 65535;      // maps beyond this are walked by stride

struct MapLoad {
    const uint16_t* d;
    unsigned W;
    __host__ __device__ unsigned operator()(int x, int y) const {
        return d[(unsigned)y * W + (unsigned)x];
    }
};

struct KeyStore {
    uint32_t* k;
    unsigned W;
    __host__ __device__ void operator()(int x, int y, uint32_t key) const {
        k[(unsigned)y * W + (unsigned)x] = key;
    }
};

// grid: x over line * segment (lines innermost), y the direction, z maps.
__global__ __launch_bounds__(kThreads) void fill_scan_kernel(
    const uint16_t* __restrict__ disps, int n, int W, int H, unsigned np, int S, int max_dist,
    unsigned invalid, uint32_t* __restrict__ keys) {
    const int k = (int)blockIdx.y;
    const unsigned lines = (unsigned)fl::n_lines(k, W, H);
    const unsigned segs = (unsigned)fl::n_segments(k, W, H, S);
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= lines * segs) return;   // lines * segs <= W * H + max(W, H) < 2^32
    const int line = (int)(i % lines), seg = (int)(i / lines);
    for (unsigned m = blockIdx.z; m < (unsigned)n; m += gridDim.z) {
        const MapLoad load{disps + (size_t)m * np, (unsigned)W};
        const KeyStore store{keys + ((size_t)m * fl::kDirs + (size_t)k) * np, (unsigned)W};
        fl::scan_segment<tune::kFillRing>(k, line, seg, W, H, S, max_dist, invalid, load, store);
    }
}

// keys null: max_dist = 0, a copy.
__global__ __launch_bounds__(kThreads) void fill_apply_kernel(
    const uint16_t* disps, const float* subpix, int n, int W, unsigned np, unsigned invalid,
    int min_found, int mode, const uint32_t* __restrict__ keys, uint16_t* out, float* out_sub,
    uint8_t* __restrict__ n_found) {
    const unsigned p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= np) return;
    for (unsigned m = blockIdx.y; m < (unsigned)n; m += gridDim.y) {
        const size_t base = (size_t)m * np, at = base + p;
        const unsigned s = disps[at];
        unsigned v = s;
        int found = 0;
        size_t src = at;
        bool filled = false;
        if (keys && !cc::valid(s, invalid)) {
            const uint32_t* kp = keys + (size_t)m * fl::kDirs * np + p;
            uint32_t key[fl::kDirs];
#pragma unroll
            for (int k = 0; k < fl::kDirs; k++) key[k] = kp[(size_t)k * np];
            found = fl::sort8(key);
            const int e = fl::pick(found, min_found, mode);
            if (e >= 0) {
                // a static index per case keeps the keys in registers
                uint32_t c = key[0];
#pragma unroll
                for (int q = 1; q < 4; q++) c = e == q ? key[q] : c;
                const int j = fl::key_j(c), k = fl::key_k(c);
                filled = true;
                v = fl::key_d(c);
                // the source lies in the frame: the scan met it there
                src = (size_t)((long long)at + (long long)j * (fl::dir_dy(k) * (long long)W + fl::dir_dx(k)));
            }
        }
        if (filled || out != disps) out[at] = (uint16_t)v;
        if (out_sub && (filled || out_sub != subpix)) out_sub[at] = subpix[src];
        if (n_found) n_found[at] = (uint8_t)found;
    }
}

}  // namespace

hipError_t launch_fill(Ctx& c, const uint16_t* disps, const float* subpix, int n, int W, int H,
                       uint16_t invalid, int max_dist, int min_found, int mode, int segment,
                       uint32_t* keys, uint16_t* out, float* out_sub, uint8_t* n_found) {
    const unsigned long long np64 = (unsigned long long)W * (unsigned long long)H;
    if (n < 1 || W <= 0 || H <= 0 || np64 >= (1ull << 31) || segment < 1 ||
        fl::thresholds_error(max_dist, min_found, mode) || (out_sub && !subpix) || !disps || !out ||
        (keys == nullptr) != (max_dist == 0))
        return hipErrorInvalidValue;
    const unsigned np = (unsigned)np64;
    hipError_t e = hipSuccess;
    if (keys) {
        // the most threads any direction needs
        unsigned most = 0;
        for (int k = 0; k < fl::kDirs; k++) {
            const unsigned t = (unsigned)fl::n_lines(k, W, H) * (unsigned)fl::n_segments(k, W, H, segment);
            most = t > most ? t : most;
        }
        const unsigned gz = (unsigned)n < kMaxGridZ ? (unsigned)n : kMaxGridZ;
        ScopedKernelTimer t(c, "fill_scan");
        hipLaunchKernelGGL(fill_scan_kernel, dim3((most + kThreads - 1) / kThreads, fl::kDirs, gz),
                           dim3(kThreads), 0, c.stream, disps, n, W, H, np, segment, max_dist,
                           (unsigned)invalid, keys);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const unsigned gy = (unsigned)n < kMaxGridZ ? (unsigned)n : kMaxGridZ;
    ScopedKernelTimer t(c, "fill_apply");
    hipLaunchKernelGGL(fill_apply_kernel, dim3((np + kThreads - 1) / kThreads, gy), dim3(kThreads), 0,
                       c.stream, disps, subpix, n, W, np, (unsigned)invalid, min_found, mode,
                       (const uint32_t*)keys, out, out_sub, n_found);
    return hipGetLastError();
}

}  // namespace sva
