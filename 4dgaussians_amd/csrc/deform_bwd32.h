// deform_bwd32.h -- D2 (backward-data) in its 32-row form, with BwdScratch / BwdDev, the kernel arguments every backward-data form shares.
// Included by deform.hip inside namespace fdgs, after deform_bwd_lists.h and in front of deform_bwd_ws.h.

// ------------------------------------------------------------------------------------------------ D2 backward-data
struct BwdScratch {
    float *G, *DH1, *DHID, *RH, *FEAT, *DFEAT;
    uint32_t *tile_live, *live, *chunks, *counters;   // per-tile non-zero flags and the lists tile_compact_kernel builds from them
    const uint32_t* rows;                             // ROWS kernels: the live rows (ascending, padded; row_gather_kernel); G is then the compact copy
    int Npad;
};
struct BwdDev {
    fdgs_deform_params p;
    AabbScale sc;
    BwdScratch s;
    float* d_w2[FDGS_NUM_HEADS];
    float* d_b2[FDGS_NUM_HEADS];
    int F;
    int head_slot[FDGS_NUM_HEADS];  // index of the head's dH1 slab
    int ntiles;                     // 32-Gaussian tiles (Npad / 32)
    const uint32_t* sv_hmask;       // SAVED kernels: the forward's per-lane ReLU bits of the trunk output
    const float *sv_rh, *sv_h1;     // SAVED kernels: relu(hidden) [Np][W], relu(h1) [slot][Np][W] written by the forward
    int small_heads;                // 1: dW2 of the k<=4 heads on the 4x4x1 MFMA with register-resident sums (the host always passes 1)
    unsigned long long* prof;       // development builds (-DFDGS_PROFILE_D2): per-wave cycle sums per phase
};
#ifdef FDGS_PROFILE_D2
#define D2_TICK(ph) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); prof_acc[ph] += t_ - prof_t; prof_t = t_; } while (0)
#else
#define D2_TICK(ph) do { } while (0)
#endif

// LDS of the backward kernel: per-wave transposed relu(h1) tile [32 gaussians][W + 4] (padded: conflict-free
// ds_write_b128 / ds_read_b32) + workgroup accumulators of dW2 / db2 for all five heads (59 rows), flushed to global
// memory once per (persistent) workgroup instead of once per 32 Gaussians.
template <int WT>
struct BwdLds {
    static constexpr int W = WT * 32;
    static constexpr int STRIDE = W + 4;
    static constexpr int TILE_FLOATS = 32 * STRIDE;
    static constexpr int KSUM = 59;                    // 3 + 3 + 4 + 1 + 48 output rows over the five heads
    static constexpr int ACC_W = KSUM * W;
    static constexpr int TOTAL = 4 * TILE_FLOATS + ACC_W + 64;
};
template <int NCH, int GQ>
__device__ __forceinline__ void small_dw2_steps(f32x4* acc, float sa0, float sa1, const float* lds, int stride, int lane) {
    if constexpr (GQ < 32) {
#pragma unroll
        for (int u = 0; u < NCH; u++)
            acc[u] = mfma4_bcast<(GQ & 15)>(GQ < 16 ? sa0 : sa1, lds[GQ * stride + 64 * u + lane], acc[u]);
        small_dw2_steps<NCH, GQ + 1>(acc, sa0, sa1, lds, stride, lane);
    }
}

// SAVED: the forward left features / relu(hidden) / relu(h1) behind (fdgs_deform_out::saved): no gather, no trunk, no
// recomputation of the heads' hidden layers -- the h1 tile is copied straight from memory into the (already transposed)
// LDS tile, the ReLU masks are read back from it, and `hid` never occupies registers.
// ROWS (with SAVED): the unit of work is a tile of 32 entries of the ROW LIST -- the Gaussians whose gradient row is non-zero, in ascending
// order -- instead of 32 consecutive Gaussians: G, DH1, DHID and DFEAT are indexed by list position (compact), the saved activations and
// the ReLU bits of a row are fetched through the list.  On the bench scene 12 % of the rows but 17.5 % of the 32-row tiles are live.
template <int WT, int FCH, bool SAVED, bool ROWS = false>
__global__ void __launch_bounds__(256, 1) deform_bwd_data_kernel(BwdDev d) {
    static_assert(SAVED || !ROWS, "the row-list form reads the saved activations");
    const fdgs_deform_params& p = d.p;
    constexpr int FT = (FCH + 3) / 4;
    using LD = BwdLds<WT>;
    constexpr int STRIDE = LD::STRIDE, W = WT * 32;
    __shared__ __attribute__((aligned(16))) float lds_all[LD::TOTAL];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g0 = lane & 31, h0 = lane >> 5;
    float* lds = lds_all + wave * LD::TILE_FLOATS;
    float* accW2 = lds_all + 4 * LD::TILE_FLOATS;
    float* accB2 = accW2 + LD::ACC_W;
    for (int i = threadIdx.x; i < LD::ACC_W + 64; i += 256) accW2[i] = 0.f;
    __syncthreads();
    const int F = d.F;

    // dW2 / db2 of the four k<=4 heads live in registers for the whole (persistent) kernel: 4x4x1 MFMA form, lane l register
    // i = dW2[i][64u + l] (u-th 64-feature chunk); db2 partials per lane (block b = lane/4 holds Gaussians b and 16+b)
    constexpr int NCH = W / 64;
    f32x4 sw[4][NCH];
    float sb[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        sb[q] = 0.f;
#pragma unroll
        for (int u = 0; u < NCH; u++) sw[q][u] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const bool small_on = d.small_heads != 0;
    // dW2 of the 48-row SH head: the four waves of the workgroup pool their transposed relu(h1) tiles (128 Gaussians) and
    // every wave OWNS one 32-column block of dW2 for both 32-row tiles, so its sums go into the LDS accumulator with plain
    // read-add-write instead of atomics.  (The per-wave form needed ~96 ds_add_f32 per tile to merge the waves' partial
    // sums: ~30 k cycles per tile, 9 % of the kernel, in-kernel cycle profile of round 1.)  Two workgroup barriers per tile.
    constexpr int NU = WT == 4 ? 2 : 1;            // (ot2, tb) units per wave: WT=4: (0,w),(1,w); WT=2: (w>>1, w&1)
    bool tiles_shared = false;   // another wave may still be reading this wave's tile: barrier before overwriting it
#ifdef FDGS_PROFILE_D2
    unsigned long long prof_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long prof_t = __builtin_amdgcn_s_memtime();
    const unsigned long long prof_t0 = prof_t;
#endif
#define FDGS_TV_LIST(OP) OP(0) OP(1) OP(2) OP(3) OP(4) OP(5) OP(6) OP(7) OP(8) OP(9) OP(10) OP(11) OP(12) OP(13) OP(14) OP(15)
#define FDGS_TV_DECL(j) float4 tv##j = make_float4(0.f, 0.f, 0.f, 0.f);
    FDGS_TV_LIST(FDGS_TV_DECL)
    bool tv_loaded = false;   // SAVED: the first head's relu(h1) tile of this tile was requested during the previous tile
    // the tiles to process: the live list (tiles with a non-zero gradient row, padded to whole groups of four)
    const const_u32p live_list = as_const(d.s.live);
    const int nlive4 = (int)as_const(d.s.counters)[ROWS ? 5 : 1];
    const int it_stride = gridDim.x * 4;
    // ROWS: list entry of lane g (both halves) for this wave's current / next tile, fetched a whole tile ahead
    uint32_t ridx_cur = 0u, ridx_nxt = 0u;
    if constexpr (ROWS) {
        const int it0 = blockIdx.x * 4 + wave;
        if (it0 < nlive4) ridx_nxt = d.s.rows[(size_t)it0 * 32 + (lane & 31)];
    }
    // ROWS: the LEFTOVER round split by head.  A tile keeps a wave busy for ~100 us and a launch has 4 x CUs waves: with 1 126 tiles on
    // 1 024 waves (the bench scene) the kernel takes two tile times although the second round holds 102 tiles.  When the tiles behind the
    // last full round number at most one per workgroup, workgroup b takes tile nfull + b with its FOUR waves: each wave runs a subset of
    // the heads (the 48-row SH head alone, the fifth head with the second wave), the partial dhid meet in LDS and wave 0 finishes the tile.
    unsigned all_heads = 0u, my_heads = 0u;
    int n_on = 0;
    {
        const int ord[FDGS_NUM_HEADS] = {FDGS_HEAD_SHS, FDGS_HEAD_POS, FDGS_HEAD_SCALE, FDGS_HEAD_ROT, FDGS_HEAD_OPACITY};
#pragma unroll
        for (int i = 0; i < FDGS_NUM_HEADS; i++)
            if (p.head_on[ord[i]]) {
                all_heads |= 1u << ord[i];
                if ((n_on < 4 ? n_on : 1) == wave) my_heads |= 1u << ord[i];
                n_on++;
            }
    }
    const int nfull = nlive4 / it_stride * it_stride, nleft = nlive4 - nfull;
    const bool split = ROWS && n_on > 1 && nleft > 0 && nleft <= (int)gridDim.x;
    const int n_normal = split ? nfull : nlive4;
    bool sp_pending = split && (int)blockIdx.x < nleft;
    // (list indices are made wave-uniform BEFORE they address the list: scalar loads.  As vector loads they would join the in-order
    // vmcnt queue behind the prefetched activation rows and every read of the list would wait for those.)
    for (int it = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(wave); ROWS || it < nlive4; it += it_stride) {
        bool sp = false;       // this iteration is the workgroup's tile of the split round
        if constexpr (ROWS) {
            if (it >= n_normal) {
                if (!sp_pending) break;
                sp = true; sp_pending = false;
            }
        }
        const unsigned heads_it = sp ? my_heads : all_heads;
        // (the tile-list kernels keep walking p.head_on: their register allocation is at the edge, 512 registers and 92 bytes of spills)
        auto nexth = [&](unsigned m, int cur) { if constexpr (ROWS) return next_head_m(m, cur); else return next_head(p.head_on, cur); };
        if (ROWS && sp && tiles_shared) { __syncthreads(); tiles_shared = false; }     // (a wave without a head in the split round would miss the barrier at the head top)
        // opaque per-iteration copies of the lane coordinates: keeps the (hundreds of) loop-invariant weight addresses
        // from being hoisted out of the tile loop and held in registers across it
        int g = g0, h = h0;
        asm volatile("" : "+v"(g), "+v"(h));
        const int tile = sp ? nfull + (int)blockIdx.x : (ROWS ? it : (int)live_list[it]);
        const int tile_next = !sp && it + it_stride < n_normal ? (ROWS ? it + it_stride : (int)live_list[it + it_stride]) : -1;
        if constexpr (ROWS) {
            if (sp) ridx_nxt = d.s.rows[(size_t)tile * 32 + (lane & 31)];      // (not requested ahead: one exposed round trip per launch)
            ridx_cur = ridx_nxt & ~ROW_PAD;
            if (tile_next >= 0) ridx_nxt = d.s.rows[(size_t)tile_next * 32 + (lane & 31)];
        }
        const int n0 = tile * 32;  // first Gaussian (ROWS: first list position) of this wave's tile (rows < Npad always exist in scratch)
        const int n_row = n0 + g;
        const int n = n_row < p.N ? n_row : p.N - 1;
        int hd = nexth(heads_it, -1);
        DenseIL<WT, WT, true, FwdPD<WT>::L1, false> L1;
        f32x16 hid[SAVED ? 1 : WT], dhid[WT];
        uint32_t hidmask[WT];   // SAVED: bit r of hidmask[t] = relu(hidden)[t][r] > 0
        if constexpr (!SAVED) {
            DenseTrunk<FCH, WT, 2> T0;
            T0.setup(p.w0, p.b0, F, g, h);
            T0.preload();
            L1.setup(p.w1[hd], p.b1[hd], W, W, g, h);   // at least one head is active (checked on the host)
            L1.preload();
            float q[4], xyz[3];
            load_query(p, d.sc, n, q, xyz);
            f32x16 feat[FT];
#pragma unroll
            for (int t = 0; t < FT; t++) feat[t] = zero16();
            gather_features<FCH>(p, q, h, feat);
#pragma unroll
            for (int j = 0; j < FCH; j++)
                *reinterpret_cast<float4*>(d.s.FEAT + (size_t)n_row * F + 8 * j + 4 * h) =
                    make_float4(feat[j / 4][4 * (j % 4)], feat[j / 4][4 * (j % 4) + 1], feat[j / 4][4 * (j % 4) + 2], feat[j / 4][4 * (j % 4) + 3]);
            D2_TICK(0);
            T0.run(feat, hid, h);
            relu_inplace<WT>(hid);
            store_il<WT>(d.s.RH + (size_t)n_row * W, hid, h);
            D2_TICK(1);
        } else {
            (void)n;
            // (sixteen 16-byte loads of the saved relu(hidden) row used to be spilled one by one here: sixteen serialised
            // HBM round trips per tile; the forward now leaves the bits behind in this lane layout)
            // (ROWS: the bits of list entry g sit in the word quadruple of its own Gaussian: tile r / 32, lane (r % 32, h))
            const uint4 hm = reinterpret_cast<const uint4*>(d.sv_hmask)[ROWS ? (size_t)(ridx_cur >> 5) * 64 + 32 * h + (ridx_cur & 31u) : (size_t)tile * 64 + lane];
            const uint32_t hmw[4] = {hm.x, hm.y, hm.z, hm.w};
#pragma unroll
            for (int t = 0; t < WT; t++) hidmask[t] = hmw[t];
        }
        // SAVED: the relu(h1) tile of the NEXT head to process is fetched one head ahead (64 registers), under the long
        // transposed product of the current one -- the kernel is otherwise HBM-latency bound on these 16-KB tiles
        // (sixteen named registers quadruples, not an array: an array carried across the head loop is "promoted" to LDS by
        // the compiler's alloca pass instead of being scalarised)
#if defined(FDGS_NT_LOAD) && FDGS_NT_LOAD      // (development variant: the saved rows are read once)
#define FDGS_TV_LOAD(j) if (j < WT * 4) { typedef float v4nt_ __attribute__((ext_vector_type(4))); \
        const v4nt_ t_ = __builtin_nontemporal_load(reinterpret_cast<const v4nt_*>(tsrc + (j * 64 + lane))); tv##j = make_float4(t_.x, t_.y, t_.z, t_.w); }
#else
#define FDGS_TV_LOAD(j) if (j < WT * 4) tv##j = tsrc[j * 64 + lane];
#endif
        // ROWS: float4 j * 64 + lane of the tile is columns 4 lc4 .. of list entry j * RPL + lrow: that entry's row of the head's slab (tslab).
        // (lrow / lc4 come from the per-head opaque copies of the lane coordinates: derived from the plain lane id they are loop
        // invariants, and the compiler keeps -- and spills -- one select index and one column offset per request)
#define FDGS_TV_LOAD_ROWS(j) if (j < WT * 4) { \
        const uint32_t r_ = (uint32_t)__shfl((int)ridx_sel, j * (256 / W) + lrow_, 64) & ~ROW_PAD; \
        tv##j = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(tslab) + (r_ * (uint32_t)(W * 4) + coff_)); }
#define FDGS_TV_ROWS_COORDS const int l64_ = 32 * h + g, lrow_ = l64_ / (W / 4); const uint32_t coff_ = (uint32_t)(l64_ % (W / 4)) * 16u;
#define FDGS_TV_STORE(j) if (j < WT * 4) { const int e4 = j * 64 + lane, row = e4 / (W / 4), c4 = e4 - row * (W / 4); \
                                          *reinterpret_cast<float4*>(lds + row * STRIDE + 4 * c4) = tv##j; }
        if constexpr (SAVED) {
            if (!tv_loaded && (!ROWS || hd < FDGS_NUM_HEADS)) {
                if constexpr (ROWS) {
                    const float* tslab = d.sv_h1 + (size_t)d.head_slot[hd] * d.s.Npad * W;
                    const uint32_t ridx_sel = ridx_cur;
                    FDGS_TV_ROWS_COORDS
                    FDGS_TV_LIST(FDGS_TV_LOAD_ROWS)
                } else {
                    const float4* tsrc = reinterpret_cast<const float4*>(d.sv_h1 + ((size_t)d.head_slot[hd] * d.s.Npad + n0) * W);
                    FDGS_TV_LIST(FDGS_TV_LOAD)
                }
            }
        }
        // SAVED: request the relu(h1) rows that are needed NEXT (next head of this tile, or the first head of this wave's
        // next tile) as soon as the 64 staging registers are free, i.e. right after they were copied to LDS -- a whole head
        // iteration ahead.  (Requested just before B1.run they sat in front of B1's operand ring in the in-order load
        // queue and every head paid their HBM latency at its first MFMA: 21 k instead of 18 k cycles per head.)
        auto request_next_rows = [&](int cur_hd) {
            if constexpr (SAVED) {
                int nx = nexth(heads_it, cur_hd);
                int nn0 = n0;
                const bool wrap = nx >= FDGS_NUM_HEADS;
                if (wrap) { nx = nexth(all_heads, -1); nn0 = tile_next * 32; }
                const bool have = !wrap || tile_next >= 0;
                tv_loaded = have && wrap;   // "this wave's next tile finds its first rows already requested"
                if (have) {
                    if constexpr (ROWS) {
                        const float* tslab = d.sv_h1 + (size_t)d.head_slot[nx] * d.s.Npad * W;
                        const uint32_t ridx_sel = wrap ? ridx_nxt : ridx_cur;
                        FDGS_TV_ROWS_COORDS
                        FDGS_TV_LIST(FDGS_TV_LOAD_ROWS)
                    } else {
                        const float4* tsrc = reinterpret_cast<const float4*>(d.sv_h1 + ((size_t)d.head_slot[nx] * d.s.Npad + nn0) * W);
                        FDGS_TV_LIST(FDGS_TV_LOAD)
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
#pragma unroll
        for (int t = 0; t < WT; t++) dhid[t] = zero16();
        const float* Grow = d.s.G + (size_t)n_row * GCOLS;

        while (hd < FDGS_NUM_HEADS) {
            asm volatile("" : "+v"(g), "+v"(h));   // no hoisting of per-layer address arithmetic out of the head loop
            const int k = head_k(hd), off = head_off(hd), row0 = head_row0(hd);
            uint32_t mask[WT];  // bit r of mask[t]: h1[t][r] > 0
            const int nt2 = k > 32 ? 2 : 1;
            // operands that depend on nothing computed in this head are requested first: the head's packed output-gradient
            // rows for the dW2 product (A-lane: output o = 32*ot2 + g, gaussian 2s+h) ...
            // (loads are unconditional -- columns past the head's k outputs lie inside the scratch buffer -- and zeroed by
            // a select: a conditional load becomes a branch that the compiler sinks to the use, exposing its latency)
            const bool small = small_on && k <= 4;
            const bool coop_e = !small && k > 32 && !(ROWS && sp);     // (split round: the four waves hold the SAME tile -- the per-wave form below)
            float ga[16];
            float sa0 = 0.f, sa1 = 0.f;   // small path: A-lane 4b+i = G[gaussian b (+16)][output i]
            if (small) {
                const float* gp = d.s.G + (size_t)(n0 + (lane >> 2)) * GCOLS + off + (lane & 3);
                sa0 = gp[0];
                sa1 = gp[(size_t)16 * GCOLS];
                sa0 = (lane & 3) < k ? sa0 : 0.f;
                sa1 = (lane & 3) < k ? sa1 : 0.f;
            } else if (ROWS ? !coop_e : k <= 32) {   // (the 48-row head takes the cooperative path and loads its rows there)
                const float* gp = d.s.G + (size_t)(n0 + h) * GCOLS + off + g;
#pragma unroll
                for (int s = 0; s < 16; s++) ga[s] = gp[(size_t)2 * s * GCOLS];
#pragma unroll
                for (int s = 0; s < 16; s++) ga[s] = g < k ? ga[s] : 0.f;
            } else {
#pragma unroll
                for (int s = 0; s < 16; s++) ga[s] = 0.f;
            }
            if constexpr (!SAVED) {
                f32x16 h1[WT];
                L1.run(hid, h1, h);
                D2_TICK(2);
#pragma unroll
                for (int t = 0; t < WT; t++) {
                    mask[t] = 0;
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        h1[t][r] = fmaxf(h1[t][r], 0.f);
                        mask[t] |= (h1[t][r] > 0.f ? 1u : 0u) << r;
                    }
                }
                // transposed copy relu(h1)[gaussian][feature] for the dW2 product
                if (tiles_shared) { __syncthreads(); tiles_shared = false; }
                store_il<WT>(lds + g * STRIDE, h1, h);
            } else {
                // the saved relu(h1) rows of this tile are 32 x W contiguous floats: copy them, lane-consecutive, into the
                // padded LDS tile [gaussian][W + 4]; then every lane reads its own Gaussian's row back for the ReLU mask
                if (tiles_shared) { __syncthreads(); tiles_shared = false; }
                FDGS_TV_LIST(FDGS_TV_STORE)
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_wave_barrier();
                D2_TICK(0);
#pragma unroll
                for (int t = 0; t < WT; t++) mask[t] = 0;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const AVec<WT> v = ldv<WT>(lds + g * STRIDE + WT * rho(r, h));
#pragma unroll
                    for (int t = 0; t < WT; t++) mask[t] |= (v.v[t] > 0.f ? 1u : 0u) << r;
                }
                if (ROWS ? !coop_e : !(!small && k > 32)) request_next_rows(hd);   // (the cooperative SH block needs the registers first)
                D2_TICK(2);
            }
            DenseT<WT, WT, true, 4> B1;
            const float* w2p = p.w2[hd] + WT * g;
            const int nsteps = (k + 1) >> 1;
            auto ldA = [&](int s) { int o = 2 * s + h; o = o < k ? o : k - 1; return ldv<WT>(w2p + (size_t)o * W); };
            // (raw loads: the o < k select is applied where the value is consumed -- a select next to the request would wait
            // for it, and with the next tile rows queued in front of it that wait is an HBM round trip)
            auto ldB = [&](int s) { return Grow[off + 2 * s + h]; };
            auto selB = [&](float v, int s) { return 2 * s + h < k ? v : 0.f; };
            AVec<WT> a0, a1, a2;
            float b0, b1, b2;
            auto early_requests = [&]() {
                B1.setup(p.w1[hd], W, W, g, h);
                B1.preload();
                a0 = ldA(0); a1 = ldA(1 < nsteps ? 1 : 0); a2 = ldA(2 < nsteps ? 2 : 0);
                b0 = ldB(0); b1 = ldB(1 < nsteps ? 1 : 0); b2 = ldB(2 < nsteps ? 2 : 0);   // steps >= nsteps are never consumed
            };
            const bool coop = ROWS ? coop_e : (!small && k > 32);
            if (!coop) early_requests();   // (the cooperative SH block needs the registers: requests follow it)
            __builtin_amdgcn_sched_barrier(0);   // keep these requests ahead of the dW2 block
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            D2_TICK(3);
            // ---- dW2[o][in] += sum_g G[g][o] * relu(h1)[g][in];  db2[o] += sum_g G[g][o]
            if (small) {
                // one 4x4x1 MFMA per (Gaussian, 64-feature chunk): B-lane l = relu(h1)[gaussian][64u + l] straight from
                // the transposed tile, A = the Gaussian's k gradient values broadcast from block gq%16 of sa0/sa1
                auto small_dw2 = [&](f32x4* acc, float& bsum) {
                    bsum += sa0 + sa1;
                    small_dw2_steps<NCH, 0>(acc, sa0, sa1, lds, STRIDE, lane);
                };
                if (hd == FDGS_HEAD_POS) small_dw2(sw[0], sb[0]);
                else if (hd == FDGS_HEAD_SCALE) small_dw2(sw[1], sb[1]);
                else if (hd == FDGS_HEAD_ROT) small_dw2(sw[2], sb[2]);
                else small_dw2(sw[3], sb[3]);
            }
            if (coop) {
                D2_TICK(4);
                __syncthreads();                                   // all four tiles of the workgroup are written
                D2_TICK(1);
                // first Gaussians of the workgroup's four tiles (entries it - wave .. + 3 of the live list)
                int wgn0[4];
#pragma unroll
                for (int c = 0; c < 4; c++) wgn0[c] = (ROWS ? (it & ~3) + c : (int)live_list[(it & ~3) + c]) * 32;
#pragma unroll
                for (int j = 0; j < NU; j++) {
                    const int ot2 = WT == 4 ? j : (wave >> 1), tb = WT == 4 ? wave : (wave & 1);
                    const int o = ot2 * 32 + g;
                    // (a uniform 64-bit base per tile + ONE 32-bit lane offset for all tiles and steps: SGPR-base addressing.  Written as
                    // `gp[(wgn0[c] + 2 s) * GCOLS]` the 64 requests took a 64-bit vector address each: +300 bytes of spills per lane,
                    // and the spill reloads wait in the in-order vmcnt queue behind the prefetched activation rows)
                    const uint32_t gvo = (uint32_t)((h * GCOLS + off + o) * 4);
                    auto gld = [&](int c, int s) {
                        const char* base = reinterpret_cast<const char*>(d.s.G) + (size_t)wgn0[c] * (GCOLS * 4);
                        return *reinterpret_cast<const float*>(base + (gvo + (uint32_t)(2 * s * GCOLS * 4)));
                    };
                    const float* bp = lds_all + tb * 32 + g;
                    float gq[2][16];
                    f32x16 accS = zero16();
                    float asumS = 0.f;
#pragma unroll
                    for (int s = 0; s < 16; s++) gq[0][s] = gld(0, s);
#pragma unroll
                    for (int c = 0; c < 4; c++) {                  // 4 chunks of 16 k-steps = the 4 tiles (32 Gaussians each)
                        if (c + 1 < 4) {
#pragma unroll
                            for (int s = 0; s < 16; s++) gq[(c + 1) & 1][s] = gld(c + 1, s);
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int s = 0; s < 16; s++) {
                            const float a = o < k ? gq[c & 1][s] : 0.f;
                            asumS += a;
                            accS = mfma32(a, bp[c * LD::TILE_FLOATS + (2 * s + h) * STRIDE], accS);
                        }
                    }
                    // this wave is the only writer of these cells: plain LDS read-add-write
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int orow = ot2 * 32 + rho(r, h);
                        if (orow < k) accW2[(row0 + orow) * W + tb * 32 + g] += accS[r];
                    }
                    if (tb == 0) {   // db2: one wave per row tile
                        asumS += __shfl_xor(asumS, 32, 64);
                        if (h == 0 && o < k) accB2[row0 + o] += asumS;
                    }
                }
                tiles_shared = true;
                D2_TICK(10);
                request_next_rows(hd);
                early_requests();
                D2_TICK(11);
            }
            for (int ot2 = 0; ot2 < ((small || coop) ? 0 : nt2); ot2++) {
                const int o = ot2 * 32 + g;
                if (ot2 > 0) {
                    const float* gp = d.s.G + (size_t)(n0 + h) * GCOLS + off + o;
#pragma unroll
                    for (int s = 0; s < 16; s++) ga[s] = gp[(size_t)2 * s * GCOLS];
#pragma unroll
                    for (int s = 0; s < 16; s++) ga[s] = o < k ? ga[s] : 0.f;
                }
                float asum = 0.f;
#pragma unroll
                for (int s = 0; s < 16; s++) asum += ga[s];
                asum += __shfl_xor(asum, 32, 64);
                const int kk = k - ot2 * 32;  // valid rows of this 32-row output tile
                if (h == 0 && g < kk) atomicAdd(&accB2[row0 + ot2 * 32 + g], asum);
                D2_TICK(10);
#pragma unroll
                for (int tb = 0; tb < WT; tb += 2) {   // two feature tiles at a time: 32 accumulator registers
                    f32x16 acc0 = zero16(), acc1 = zero16();
#pragma unroll
                    for (int s = 0; s < 16; s++) {
                        acc0 = mfma32(ga[s], lds[(2 * s + h) * STRIDE + tb * 32 + g], acc0);
                        acc1 = mfma32(ga[s], lds[(2 * s + h) * STRIDE + (tb + 1) * 32 + g], acc1);
                    }
                    D2_TICK(11);
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int orow = rho(r, h);
                        if (orow < kk) {
                            atomicAdd(&accW2[(row0 + ot2 * 32 + orow) * W + tb * 32 + g], acc0[r]);
                            atomicAdd(&accW2[(row0 + ot2 * 32 + orow) * W + (tb + 1) * 32 + g], acc1[r]);
                        }
                    }
                }
            }
            D2_TICK(4);
            // ---- dh1 = W2^T G_head, masked by relu'(h1)
            f32x16 dh1[WT];
#pragma unroll
            for (int t = 0; t < WT; t++) dh1[t] = zero16();
            if (k > 32) {
                // the 48-output head: 24 k-steps, fully unrolled with a 6-deep operand ring (a 3-deep rotating ring left the
                // MFMAs waiting on L2 for most steps: 12 % of the kernel in the cycle profile)
                constexpr int PDH = 6, NSH = 24;
                AVec<WT> ra[PDH];
                float rb[PDH];
                ra[0] = a0; ra[1] = a1; ra[2] = a2; rb[0] = b0; rb[1] = b1; rb[2] = b2;
#pragma unroll
                for (int s = 3; s < PDH; s++) { ra[s] = ldA(s); rb[s] = ldB(s); }
#pragma unroll
                for (int s = 0; s < NSH; s++) {
                    const AVec<WT> a = ra[s % PDH];
                    const float b = selB(rb[s % PDH], s);
                    if (s + PDH < NSH) { ra[s % PDH] = ldA(s + PDH); rb[s % PDH] = ldB(s + PDH); }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int t = 0; t < WT; t++) dh1[t] = mfma32(a.v[t], b, dh1[t]);
                }
            } else {
                for (int s = 0; s < nsteps; s++) {
                    const AVec<WT> a = a0;
                    const float b = selB(b0, s);
                    a0 = a1; b0 = b1; a1 = a2; b1 = b2;
                    if (s + 3 < nsteps) { a2 = ldA(s + 3); b2 = ldB(s + 3); }
#pragma unroll
                    for (int t = 0; t < WT; t++) dh1[t] = mfma32(a.v[t], b, dh1[t]);
                }
            }
            D2_TICK(5);
            float* slab = d.s.DH1 + (size_t)d.head_slot[hd] * d.s.Npad * W;
#pragma unroll
            for (int t = 0; t < WT; t++)
#pragma unroll
                for (int r = 0; r < 16; r++) dh1[t][r] = ((mask[t] >> r) & 1u) ? dh1[t][r] : 0.f;
            // through the (now idle) LDS tile when no other wave can still be reading it: 32 contiguous rows, 1 KB per store
            if (!tiles_shared) store_tile_coalesced<WT>(lds, slab + (size_t)n0 * W, dh1, g, h, lane);
            else store_il<WT>(slab + (size_t)n_row * W, dh1, h);
            D2_TICK(6);
            // ---- dhid += W1^T dh1
            B1.run(dh1, dhid);
            __builtin_amdgcn_wave_barrier();
            D2_TICK(7);
            hd = nexth(heads_it, hd);
            if constexpr (!SAVED) {
                if (hd < FDGS_NUM_HEADS) { L1.setup(p.w1[hd], p.b1[hd], W, W, g, h); L1.preload(); }
            }
        }
        if constexpr (ROWS) {
            if (sp) {      // the waves' partial dhid meet in their (idle) LDS tiles; wave 0 sums them and finishes the tile
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int t = 0; t < WT; t++)
#pragma unroll
                    for (int r = 0; r < 16; r++) lds[(t * 16 + r) * 64 + lane] = dhid[t][r];
                __syncthreads();
                if (wave != 0) continue;      // (the last iteration of this workgroup: everybody meets again at the flush below)
                const int nsets = n_on < 4 ? n_on : 4;
                for (int w = 1; w < nsets; w++) {
#pragma unroll
                    for (int t = 0; t < WT; t++)
#pragma unroll
                        for (int r = 0; r < 16; r++) dhid[t][r] += lds_all[w * LD::TILE_FLOATS + (t * 16 + r) * 64 + lane];
                }
            }
        }
        // relu'(hidden), store for the trunk weight gradient, then dfeat = W0^T dhid
        DenseT<WT, FT, false, 16> B0;   // one dword per k-step and only FT MFMAs behind it: a deep ring hides the L2 latency
        B0.setup(p.w0, F, F, g, h);
        B0.preload();
#pragma unroll
        for (int t = 0; t < WT; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                bool pos;
                if constexpr (SAVED) pos = (hidmask[t] >> r) & 1u; else pos = hid[t][r] > 0.f;
                dhid[t][r] = pos ? dhid[t][r] : 0.f;
            }
        store_il<WT>(d.s.DHID + (size_t)n_row * W, dhid, h);
        f32x16 dfeat[FT];
#pragma unroll
        for (int t = 0; t < FT; t++) dfeat[t] = zero16();
        B0.run(dhid, dfeat);
#pragma unroll
        for (int j = 0; j < FCH; j++)
            *reinterpret_cast<float4*>(d.s.DFEAT + (size_t)n_row * F + 8 * j + 4 * h) =
                make_float4(dfeat[j / 4][4 * (j % 4)], dfeat[j / 4][4 * (j % 4) + 1], dfeat[j / 4][4 * (j % 4) + 2],
                            dfeat[j / 4][4 * (j % 4) + 3]);
        D2_TICK(8);
    }
#ifdef FDGS_PROFILE_D2
    if (d.prof && lane == 0) {
        unsigned long long* out = d.prof + (size_t)(blockIdx.x * 4 + wave) * 12;
        for (int i = 0; i < 9; i++) out[i] = prof_acc[i];
        out[9] = __builtin_amdgcn_s_memtime() - prof_t0;
        out[10] = prof_acc[10]; out[11] = prof_acc[11];
    }
#endif
    // the register-resident sums of the k<=4 heads join the LDS accumulators
    if (small_on) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int kq = head_k(q), r0 = head_row0(q);
            if (!p.head_on[q]) continue;
#pragma unroll
            for (int u = 0; u < NCH; u++)
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (i < kq) atomicAdd(&accW2[(r0 + i) * W + 64 * u + lane], sw[q][u][i]);
            float v = sb[q];   // lanes with equal (lane & 3): sum over the 16 blocks
            v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
            if (lane < kq) atomicAdd(&accB2[r0 + lane], v);
        }
    }
    // flush the workgroup's dW2 / db2 sums
    __syncthreads();
    for (int hd = 0; hd < FDGS_NUM_HEADS; hd++) {
        if (!p.head_on[hd]) continue;
        const int k = head_k(hd), row0 = head_row0(hd);
        for (int i = threadIdx.x; i < k * W; i += 256) {
            const float v = accW2[row0 * W + i];
            if (v != 0.f) atomicAdd(&d.d_w2[hd][i], v);
        }
        if ((int)threadIdx.x < k && accB2[row0 + threadIdx.x] != 0.f) atomicAdd(&d.d_b2[hd][threadIdx.x], accB2[row0 + threadIdx.x]);
    }
}
