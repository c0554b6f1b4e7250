// wta_hv_tile.inc -- the text of wta_hv.hip's kernel, included there once per
// instance: the plain one (SVA_WTAHV_CONF 0, wta_hv_kernel) and the confidence
// one (SVA_WTAHV_CONF 1, wta_hv_conf_kernel, DESIGN.md §2.4b).  The plain
// instance must compile to the instructions it had before the confidence one
// existed (tools/isa_same.py), and a shared inlined body did not: it changed
// the register allocation of every instance.  So the confidence parts are
// preprocessor blocks, and with SVA_WTAHV_CONF 0 the kernel is token for token
// the one it was.  This is a product route chosen by the entry point
// (launch_wta_hv's cf), not a build switch.
template <int DPL, int TYL, bool PAD, bool PAIR, bool MN>
#if SVA_WTAHV_CONF
__global__ __launch_bounds__(TB, tune::kWtahvMinWaves) void wta_hv_conf_kernel(
    const uint8_t* __restrict__ C, const uint8_t* __restrict__ L4, const uint8_t* __restrict__ CK,
    const uint8_t* __restrict__ CKV, const uint8_t* __restrict__ MNP, WtaHvGeom g,
    uint16_t* __restrict__ disp, float* __restrict__ sub, ConfOut cf) {
#else
__global__ __launch_bounds__(TB, tune::kWtahvMinWaves) void wta_hv_kernel(const uint8_t* __restrict__ C,
                                                    const uint8_t* __restrict__ L4,
                                                    const uint8_t* __restrict__ CK,
                                                    const uint8_t* __restrict__ CKV,
                                                    const uint8_t* __restrict__ MNP, WtaHvGeom g,
                                                    uint16_t* __restrict__ disp,
                                                    float* __restrict__ sub) {
#endif
    constexpr int NW = DPL / 4, NP = DPL / 2;
    constexpr int TY = 1 << TYL;        // tile rows = checkpoint segment (rows and columns)
    constexpr int kPfVol = pf_vol<DPL, PAIR>();
    constexpr bool PIN = tune::kWtahvPinRowMin != 0;     // row_min_u32<PIN>

    constexpr int SPR = TW / TY;        // phase H: row segments per tile row
    static_assert(TY <= TW && TW % TY == 0, "tile rows must divide 16");
    // a batch of frames (DESIGN.md §4.10): frame f's planes follow frame f-1's
    const unsigned f = blockIdx.x / (unsigned)g.tiles;
    const unsigned tb = blockIdx.x - f * (unsigned)g.tiles;
    const int tx = (int)(tb % (unsigned)g.ntx);
    const int ty = (int)(tb / (unsigned)g.ntx);
    constexpr int NV = PAIR ? 2 : 4;                    // diagonal volumes read
    static_assert(!MN || TY == kMinimaSeg, "path minima: 8-pixel segments");
    C += (size_t)f * g.vol;
    L4 += (size_t)f * NV * g.vol;
    CK += (size_t)f * 2 * g.hck;
    CKV += (size_t)f * 2 * g.vck;
    disp += (size_t)f * (size_t)g.W * (size_t)g.H;
    if (sub) sub += (size_t)f * (size_t)g.W * (size_t)g.H;
#if SVA_WTAHV_CONF
    // the cost planes are [frames][H][W] like disp (uniqueness and invalid:
    // one value per launch)
    if (cf.cost_min) cf.cost_min += (size_t)f * (size_t)g.W * (size_t)g.H;
    if (cf.cost_second) cf.cost_second += (size_t)f * (size_t)g.W * (size_t)g.H;
#endif
    const int slot = (int)(threadIdx.x >> 4);
    const int k = (int)(threadIdx.x & 15);
    const int W = g.W, H = g.H;
    const unsigned uD = (unsigned)g.D, uW = (unsigned)W;
    const unsigned P1 = (unsigned)g.P1, P2 = (unsigned)g.P2;
    const int x0 = tx * TW, y0 = ty * TY;
    const int nx = W - x0 < TW ? W - x0 : TW;       // tile columns inside the image (uniform)
    const int ny = H - y0 < TY ? H - y0 : TY;       // tile rows inside the image (uniform)
    const unsigned lane_d = (unsigned)(k * DPL);
    const rsrc_t rC = make_rsrc(C, g.vol);
    unsigned padm[NP];
#pragma unroll
    for (int j = 0; j < NP; j++) {
        const int dl = k * DPL + pair_d<DPL>(j, 0), dh = k * DPL + pair_d<DPL>(j, 1);
        padm[j] = PAD ? ((dl >= g.dreal ? 0x0000ffffu : 0u) | (dh >= g.dreal ? 0xffff0000u : 0u))
                      : 0u;
    }

    // V = L_2 + L_3 per tile pixel, [pixel = r * TW + c][lane k][NP pairs]:
    // each 16-lane row reads / writes 16 consecutive NP-dword chunks.
    // vw(p) = the word of pair p inside a pixel block: word p % 4 of the
    // lane's first or second 16-byte chunk (one b128 access each).
    __shared__ unsigned vsum[TY * TW * 16 * NP];
    const int vb0 = k * NP, vb1 = k * NP + 4;
    auto vw = [&](int p) -> int { return (p < 4 ? vb0 : vb1) + (p & 3); };

    // phase V: column x0 + slot; phase H: row hr, columns [hx, hx + TY)
    const bool vcol = slot < nx;
    const int hr = slot / SPR, hseg = slot % SPR;
    const int hx = x0 + hseg * TY;                    // first column of the row segment
    const int nh = W - hx < TY ? W - hx : TY;         // its pixels inside the image
    const bool hrow = hr < ny && nh > 0;
    const unsigned xv = (unsigned)(x0 + slot), yh = (unsigned)(y0 + hr);

    // Both phases' cost words are loaded up front: the tile's column slice for
    // phase V and its row slice for phase H (the same bytes, L2-hot the second
    // time).
    Words<NW> cv[TY], ch[TY];
#pragma unroll
    for (int r = 0; r < TY; r++)
        cv[r] = bload<NW>(rC, ((unsigned)(y0 + r) * uW + xv) * uD + lane_d);
    auto load_row = [&]() {
#pragma unroll
        for (int j = 0; j < TY; j++)
            ch[j] = bload<NW>(rC, (yh * uW + (unsigned)(hx + j)) * uD + lane_d);
    };
    load_row();
    // the slot's entering minima: phase V's column segment (directions 2, 3)
    // and phase H's row segment (0, 1), 8 bytes each, the same in all 16 lanes
    Words<2> mv[2] = {}, mh[2] = {};
    if constexpr (MN) {
        const unsigned hmn = (unsigned)H * (unsigned)g.nsx * (unsigned)kMinimaSeg;
        const unsigned vmn = (unsigned)g.nty * uW * (unsigned)kMinimaSeg;
        const unsigned vo = ((unsigned)ty * uW + xv) * (unsigned)kMinimaSeg;
        const unsigned ho = ((unsigned)(y0 + (slot / SPR)) * (unsigned)g.nsx +
                             (unsigned)((x0 + (slot % SPR) * TY) >> TYL)) * (unsigned)kMinimaSeg;
#pragma unroll
        for (int d = 0; d < 2; d++) {
            mv[d] = bload<2>(make_rsrc(MNP + 2 * (size_t)hmn + (size_t)d * vmn, vmn), vo);
            mh[d] = bload<2>(make_rsrc(MNP + (size_t)d * hmn, hmn), ho);
        }
    }
    // m of step i (MN), else the running minimum the last step left
    auto given_m = [](unsigned& m, const Words<2>& w, int i) {
        if constexpr (MN) m = minima_byte(w, i);
    };

    auto zero_state = [](unsigned (&A)[NP], unsigned& m) {
#pragma unroll
        for (int j = 0; j < NP; j++) A[j] = 0u;   // L(q) = 0, m = 0  =>  L = C
        m = 0u;
    };
    unsigned Aa[NP], Ab[NP], ma, mb;
    Edges ea, eb;
    // ---- phase V: down (direction 2), then up (direction 3) ----------------
    if (vcol) {
        if (ty > 0)
            load_state<DPL, PAD, PIN, MN>(make_rsrc(CKV, g.vck), ((unsigned)(ty - 1) * uW + xv) * uD + lane_d,
                                 Aa, ma, padm);
        else
            zero_state(Aa, ma);
        if (y0 + TY < H)
            load_state<DPL, PAD, PIN, MN>(make_rsrc(CKV + g.vck, g.vck),
                                 ((unsigned)(ty + 1) * uW + xv) * uD + lane_d, Ab, mb, padm);
        else
            zero_state(Ab, mb);
        // The down pass keeps each pixel's L_2 as the step's u16 pairs, so
        // V = L_2 + L_3 is NP packed adds.
        auto keep = [&](unsigned (&dst)[NP], const unsigned (&A)[NP]) {
#pragma unroll
            for (int q = 0; q < NP; q++) dst[q] = A[q];
        };
        auto put_v = [&](int r, const unsigned (&ld)[NP], const unsigned (&Au)[NP],
                         const unsigned (&cw)[NW]) {
            unsigned V[NP];
#pragma unroll
            for (int p = 0; p < NP; p++) V[p] = ld[p] + Au[p];   // L_2 + L_3 (<= 510 per half)
            if constexpr (PAIR) {
                // + 4C, what the two pair sums leave out (<= 1020 per half: no carry)
                unsigned c4[NP];
                words_to_pairs<DPL>(cw, c4);
#pragma unroll
                for (int p = 0; p < NP; p++) V[p] += c4[p] << 2;
            }
            unsigned* dst = &vsum[(r * TW + slot) * 16 * NP];
#pragma unroll
            for (int p = 0; p < NP; p++) dst[vw(p)] = V[p];
        };
        unsigned LD[TY][NP];
        for_seq<TY>([&](auto I) {
            constexpr int i = decltype(I)::value;
            unsigned ow[NW];
            if (i < ny) {
                given_m(ma, mv[0], i);
                sgm_step<DPL, PIN, MN>(cv[i].w, Aa, ma, ow, P1, P2, ea);
                keep(LD[i], Aa);
            }
        });
        for_seq<TY>([&](auto Q) {
            constexpr int r = TY - 1 - decltype(Q)::value;
            if (r < ny) {
                unsigned lu[NW];
                given_m(mb, mv[1], TY - 1 - r);
                sgm_step<DPL, PIN, MN>(cv[r].w, Ab, mb, lu, P1, P2, eb);
                put_v(r, LD[r], Ab, cv[r].w);
            }
        });
    }
    // phase H's first global loads (checkpoints, diagonal volumes) go out
    // before the barrier
    const int hs = hx >> TYL;                          // the row segment's index
    const unsigned ckrow = yh * (unsigned)g.nsx;
    Words<NW> ckw[2];
    rsrc_t rV[NV];
#pragma unroll
    for (int r = 0; r < NV; r++) rV[r] = make_rsrc(L4 + (size_t)r * g.vol, g.vol);
    Words<NW> rv[kPfVol][NV];
    auto issue = [&](int s, int j) {
        const unsigned off = (yh * uW + (unsigned)(hx + j)) * uD + lane_d;
#pragma unroll
        for (int r = 0; r < NV; r++) rv[s][r] = bload<NW, 2>(rV[r], off);   // last use: nt
    };
    auto issue_first = [&]() {
        // (words outside the image are never used: the first / last segment
        // starts from zero state)
        ckw[0] = bload<NW>(make_rsrc(CK, g.hck), (ckrow + (unsigned)(hs - 1)) * uD + lane_d);
        ckw[1] = bload<NW>(make_rsrc(CK + g.hck, g.hck), (ckrow + (unsigned)(hs + 1)) * uD + lane_d);
#pragma unroll
        for (int q = 0; q < kPfVol && q < TY; q++) issue(q, TY - 1 - q);
    };
    if (hrow) issue_first();
    __syncthreads();

    // ---- phase H: left-to-right (direction 0), then right-to-left (1) with
    // the sum and the WTA per pixel
    if (!hrow) return;                                 // whole 16-lane row leaves together
    if (hs > 0) state_from_words<DPL, PAD, PIN, MN>(ckw[0], Aa, ma, padm);
    else zero_state(Aa, ma);
    // L_0 of the segment's pixels, kept like phase V's L_2 (u16 pairs)
    unsigned LF[TY][NP];
    for_seq<TY>([&](auto I) {
        constexpr int i = decltype(I)::value;
        unsigned ow[NW];
        if (i < nh) {
            given_m(ma, mh[0], i);
            sgm_step<DPL, PIN, MN>(ch[i].w, Aa, ma, ow, P1, P2, ea);
#pragma unroll
            for (int q = 0; q < NP; q++) LF[i][q] = Aa[q];
        }
    });
    if (hx + TY < W) state_from_words<DPL, PAD, PIN, MN>(ckw[1], Aa, ma, padm);
    else zero_state(Aa, ma);
    unsigned dres = 0u, sm = 0u, s0 = 0u;
#if SVA_WTAHV_CONF
    unsigned s2 = 0xffffu;                             // cost_second of lane k's pixel
#endif
    const bool want_sub = sub != nullptr;
    unsigned dpair[NP];                                // each pair's two d, for wta_pick_key_perm
#pragma unroll
    for (int j = 0; j < NP; j++)
        dpair[j] = (lane_d + (unsigned)pair_d<DPL>(j, 0)) | ((lane_d + (unsigned)pair_d<DPL>(j, 1)) << 16);
    unsigned* const vrow = &vsum[(hr * TW + hseg * TY) * 16 * NP];   // the segment's V blocks
    for_seq<TY>([&](auto Q) {
        constexpr int q = decltype(Q)::value, j = TY - 1 - q, s = q % kPfVol;
        if (j < nh) {
            unsigned ow[NW];
            given_m(ma, mh[1], q);
            sgm_step<DPL, PIN, MN>(ch[j].w, Aa, ma, ow, P1, P2, ea);
            unsigned* const vpix = vrow + j * 16 * NP;                     // this pixel's V
            unsigned S[NP];
#pragma unroll
            for (int p = 0; p < NP; p++) S[p] = vpix[vw(p)] + Aa[p];   // V + L_1
#pragma unroll
            for (int p = 0; p < NP; p++) S[p] += LF[j][p];     // + L_0
#pragma unroll
            for (int r = 0; r < NV; r++) unpack_add<NW>(rv[s][r].w, S);
            if constexpr (PAD) {
#pragma unroll
                for (int p = 0; p < NP; p++) S[p] |= padm[p];
            }
            // S(d*-1) and S(d*+1) go through LDS: every lane writes its S
            // pairs over the pixel's V block, which nothing reads again; as
            // u16 the block is S in the state's pair layout.  The owning lane
            // reads the two neighbours once after the row segment (below).
            const unsigned best = wta_pick_key_perm<DPL, PIN && tune::kWtahvPinWta>(S, dpair);
            const int ds = (int)(best & 0xffffu);
            if (want_sub) {
#pragma unroll
                for (int p = 0; p < NP; p++) vpix[vw(p)] = S[p];
            }
            dres = k == j ? (unsigned)ds : dres;
            s0 = k == j ? best >> 16 : s0;
#if SVA_WTAHV_CONF
            const unsigned sec = wta_second_key_perm<DPL, PIN && tune::kWtahvPinWta>(
                S, dpair, (unsigned)ds, lane_d);
            s2 = k == j ? sec : s2;
#endif
        }
        if constexpr (q + kPfVol < TY) {
            __builtin_amdgcn_sched_barrier(0);
            issue(s, TY - 1 - (q + kPfVol));
            __builtin_amdgcn_sched_barrier(0);
        }
    });
    // S(d*-1), S(d*+1) of lane k's pixel (j = k) from the S its row wrote
    // over the pixel's V block (same wave: order, no barrier instruction)
    if (want_sub) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (k < nh) {
            const uint16_t* s16 = reinterpret_cast<const uint16_t*>(vrow + k * 16 * NP);
            const int ds = (int)dres;
            const int dm = ds > 0 ? ds - 1 : 0, dp = ds + 1 < 16 * DPL ? ds + 1 : ds;
            // u16 of disparity d: half half_of(d % DPL) of pair pair_of(d % DPL) of lane d / DPL
            auto at = [&](int d) {
                const int kk = d / DPL, pp = pair_of<DPL>(d % DPL), hh = half_of<DPL>(d % DPL);
                return (unsigned)s16[2 * (kk * NP + pp) + hh];
            };
            sm = at(dm) | (at(dp) << 16);
        }
    }
    if (k < nh) {
        const size_t at = (size_t)yh * (size_t)W + (size_t)(hx + k);
#if SVA_WTAHV_CONF
        // (the planes were advanced to this block's frame above.)  They keep
        // their values where the filter rejects the pixel.
        if (cf.cost_min) cf.cost_min[at] = (uint16_t)s0;
        if (cf.cost_second) cf.cost_second[at] = (uint16_t)s2;
        const bool rej = conf_reject(s0, s2, cf.uniqueness);
        disp[at] = rej ? (uint16_t)cf.invalid : (uint16_t)(g.dmin + (int)dres);
        if (want_sub) {
            const float v = subpixel(g.dmin, (int)dres, g.dreal, sm & 0xffffu, s0, sm >> 16);
            sub[at] = rej ? __builtin_nanf("") : v;
        }
#else
        disp[at] = (uint16_t)(g.dmin + (int)dres);
        if (want_sub) sub[at] = subpixel(g.dmin, (int)dres, g.dreal, sm & 0xffffu, s0, sm >> 16);
#endif
    }
}
