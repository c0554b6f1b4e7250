// cost_fuse_kernel.inc -- the fusion kernel's text, included by cost_fuse.hip
// once per visibility rule (its header comment describes the kernel).  The
// includer defines
//   SVA_FUSE_KERNEL     the kernel's name
//   SVA_FUSE_RATIOS     empty, or one more kernel argument ending in a comma
//   SVA_FUSE_LIM(i)     lim of pair i at pixel (x, y): visible at d < lim
// Text inclusion and not a template flag or a shared device function: the
// equal-baseline instances keep their kernel names and, instruction for
// instruction, the code they had before the mixed rule existed (passing the
// step struct into an inlined function moved its reads off the scalar unit).

// NC = D / 16 lanes per pixel; NM = pair-count class (n <= NM).
template <int NC, int NM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void SVA_FUSE_KERNEL(
    const uint8_t* __restrict__ volumes, size_t stride, int n, int W, int H, unsigned nlanes,
    int dmin, int dreal, FuseSteps steps, SVA_FUSE_RATIOS uint8_t* __restrict__ fused) {
    constexpr int D = NC * 16;
    __shared__ unsigned magic[33];
    if (threadIdx.x < 33) magic[threadIdx.x] = mb::mean_magic((int)threadIdx.x);
    __syncthreads();
    const unsigned lane = blockIdx.x * 256u + threadIdx.x;
    if (lane >= nlanes) return;
    const unsigned pix = lane / NC;
    const int c = (int)(lane - pix * NC);
    const int y = (int)(pix / (unsigned)W), x = (int)(pix - (unsigned)y * (unsigned)W);
    const int d0 = 16 * c;
    const unsigned off = lane * 16u;   // < W*H*D < 2^32: inside one volume

    unsigned E[4] = {0, 0, 0, 0}, O[4] = {0, 0, 0, 0}, cnt[4] = {0, 0, 0, 0};
    auto load4 = [&](int i0, v4u (&v)[4]) {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (i0 + j < n) {   // uniform
                // 64-bit and uniform; pinned to a scalar pair so that the load
                // is "scalar base + 32-bit lane offset", not a 64-bit add per lane
                uint64_t base = (uint64_t)volumes + (uint64_t)(i0 + j) * stride;
                asm("" : "+s"(base));
                v[j] = __builtin_nontemporal_load((gv4u*)(base + off));
            }
    };
    auto sum4 = [&](int i0, const v4u (&v)[4]) {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (i0 + j < n) {   // uniform
                const int lim = SVA_FUSE_LIM(i0 + j);
                const int k = lim - d0;   // visible bytes of this lane: the first k
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int kq = k - 4 * q;
                    const unsigned mask =
                        kq >= 4 ? 0xffffffffu : (kq <= 0 ? 0u : (1u << (8 * kq)) - 1u);
                    const unsigned w = v[j][q] & mask;
                    E[q] += w & 0x00ff00ffu;
                    O[q] += (w >> 8) & 0x00ff00ffu;
                    cnt[q] += mask & 0x04040404u;
                }
            }
    };
    v4u cur[4] = {}, nxt[4] = {};
    load4(0, cur);
#pragma unroll
    for (int i0 = 0; i0 < NM; i0 += 4) {
        if (i0 + 4 < NM && i0 + 4 < n) load4(i0 + 4, nxt);
        if (i0 < n) sum4(i0, cur);
#pragma unroll
        for (int j = 0; j < 4; j++) cur[j] = nxt[j];
    }

    unsigned out[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        unsigned w = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const unsigned n4 = (cnt[q] >> (8 * b)) & 0xffu;   // 4 * n = the magic's LDS offset
            const unsigned s = ((b & 1 ? O[q] : E[q]) >> (16 * (b >> 1))) & 0xffffu;
            const unsigned mg = *(const unsigned*)((const char*)magic + n4);
            const unsigned r = n4 ? mb::mean_round(2u * s + (n4 >> 2), mg) : 62u;
            w |= r << (8 * b);
        }
        out[q] = w | pad_bytes(d0 + 4 * q, dreal);
    }
    *(v4u*)(fused + off) = (v4u){out[0], out[1], out[2], out[3]};
}
