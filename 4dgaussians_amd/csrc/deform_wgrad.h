// deform_wgrad.h -- D3, the weight-gradient kernel.  Included by deform.hip inside namespace fdgs, after the backward-data kernels.

// ------------------------------------------------------------------------------------------------ D3 weight grads
// dW[m][c] += sum_n DY[n][m] * X[n][c]   (m < W rows of DY, c < ncols of X), db[m] += sum_n DY[n][m];  K = #Gaussians.
// One wave owns the WHOLE [W x ncols] product for its slice of Gaussians (16 accumulator tiles = 256 AGPRs at W = 128,
// one wave per SIMD): with the interleaved tile mapping (row m = WT*i + a, column c = WT*j + b) a k-step of two Gaussians
// needs exactly ONE 16-byte load of DY[n][WT*g ..] and ONE of X[n][WT*g ..] per lane for its 16 MFMAs -- both
// 512-byte coalesced rows, prefetched WG_PD steps ahead.  The four waves of a workgroup split the workgroup's Gaussians,
// meet in an LDS accumulator (ds_add_f32) and flush each weight once per workgroup with coalesced global atomics.
// (Round-1 kernel: one dword load per MFMA operand, 4 MFMAs per vmcnt(0) -> 36 % MFMA utilisation.)
struct WgradJob {
    const float* DY; const float* X; float* dW; float* db;
    int ldx, ncols, ldw;
    int first_block, nblocks;   // workgroups [first_block, first_block + nblocks) share the live tiles of this job evenly
};
struct WgradArgs {
    WgradJob job[FDGS_NUM_HEADS + 1];
    int njobs, Npad, W;
    const uint32_t* live;       // live-tile list (tile_compact_kernel)
    const uint32_t* counters;   // [1] = entries of the list
    const uint32_t* rows;       // ROWS kernel: the live-row list; DY is indexed by list position, X by the listed row; counters[5] = tiles of the list
};

// COLS_IL: X has exactly W columns, column mapping interleaved (vector loads); else tile mapping c = 32*b + j with
// CT = ceil(ncols/32) dword loads per k-step (the small trunk product, ncols = C*L).
// PD (8 or 16) = depth of the operand ring in k-steps: the narrow trunk products run only CT MFMAs per step, so they need a deeper
// ring than the square head products to cover the same memory latency.
// The wave walks the tiles [t_begin, t_end) of the LIVE list: a tile is 32 consecutive Gaussians = 16 k-steps, tiles need not be
// adjacent in memory (tiles whose gradient rows are all zero were dropped from the list: their products are exactly zero).
// ROWS: the tiles are 32 consecutive entries of the live-ROW list (`live` = that list): DY rows are list positions, X rows the listed Gaussians.
template <int WT, int CT, bool COLS_IL, int PD, bool ROWS>
__device__ __forceinline__ void wgrad_wave(const WgradJob& J, int W, const_u32p live, int t_begin, int t_end, float* ldsW, float* ldsB,
                                           int g, int h, int wave) {
    static_assert(16 % PD == 0, "the ring must divide a tile's 16 k-steps");
    constexpr int BV = COLS_IL ? WT : 1, NB = COLS_IL ? 1 : CT;
    f32x16 acc[WT][CT];
#pragma unroll
    for (int a = 0; a < WT; a++)
#pragma unroll
        for (int b = 0; b < CT; b++) acc[a][b] = zero16();
    float asum[WT];
#pragma unroll
    for (int a = 0; a < WT; a++) asum[a] = 0.f;
    const float* ap = J.DY + (size_t)h * W + WT * g;          // + row * W, row = first Gaussian of the k-step (even)
    const float* bp[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) {
        int col = COLS_IL ? WT * g : 32 * b + g;
        col = col < J.ncols ? col : J.ncols - 1;
        bp[b] = J.X + (ROWS ? (size_t)0 : (size_t)h * J.ldx) + col;
    }
    AVec<WT> abuf[PD];
    AVec<BV> bbuf[PD][NB];
    // slot u is consumed, THEN refilled in place with the step PD ahead; no control flow inside a tile.  (A first form copied the
    // slot, refilled it and then ran the MFMAs under `if (s < nsteps)`; the register copies at the loop back-edge and the per-step
    // branches made the wait-count pass put `vmcnt(0)` in front of the last MFMAs of EVERY step: 57 % MFMA utilisation, rocprofv3 r01h.)
    auto consume = [&](int u) {
#pragma unroll
        for (int a = 0; a < WT; a++) asum[a] += abuf[u].v[a];
#pragma unroll
        for (int a = 0; a < WT; a++)
#pragma unroll
            for (int b = 0; b < CT; b++)
                acc[a][b] = mfma32(abuf[u].v[a], COLS_IL ? bbuf[u][0].v[b] : bbuf[u][b].v[0], acc[a][b]);
    };
    auto fill = [&](int u, int row) {
        abuf[u] = ldv<WT>(ap + (size_t)row * W);
        if constexpr (ROWS) {      // (two scalar reads of the list, one select: lane half h takes entry row + h)
            const uint32_t ra = live[row] & ~ROW_PAD, rb = live[row + 1] & ~ROW_PAD;
            const uint32_t xr = h ? rb : ra;
#pragma unroll
            for (int b = 0; b < NB; b++) bbuf[u][b] = ldv<BV>(bp[b] + (size_t)xr * J.ldx);
        } else {
#pragma unroll
            for (int b = 0; b < NB; b++) bbuf[u][b] = ldv<BV>(bp[b] + (size_t)row * J.ldx);
        }
    };
    if (t_end > t_begin) {
        auto tile_row = [&](int ti) { const int tc = ti < t_end ? ti : t_end - 1; return ROWS ? tc * 32 : (int)live[tc] * 32; };      // (uniform index: scalar load)
        int cur = tile_row(t_begin), nxt = tile_row(t_begin + 1);
#pragma unroll
        for (int u = 0; u < PD; u++) fill(u, cur + 2 * u);
        for (int ti = t_begin; ti < t_end; ti++) {
            const int nxt2 = tile_row(ti + 2);      // (scalar load, consumed one tile later)
#pragma unroll
            for (int gi = 0; gi < 16 / PD; gi++) {
#pragma unroll
                for (int u = 0; u < PD; u++) {
                    consume(u);
                    __builtin_amdgcn_sched_barrier(0);
                    const int sn = gi * PD + u + PD;              // the step this slot holds next: same tile, or the next one
                    fill(u, (sn < 16 ? cur : nxt) + 2 * (sn & 15));   // (past the last tile: harmless re-load, never consumed)
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            cur = nxt; nxt = nxt2;
        }
    }
    // workgroup reduction in LDS, ldsW[m * ldl + c] with ldl = 32*CT: the four waves take turns (barrier between turns) and
    // use plain stores / read-add-writes -- ds_add_f32 runs at 0.33 lanes/clk/CU on MI355X (tools/lds_atomic_bench.hip:
    // 37x slower than ds_add_u32, ~200x slower than plain LDS traffic) and 4 x 16 k float atomics cost ~15 % of this kernel
    constexpr int LDL = 32 * CT;
    float bsum[WT];
#pragma unroll
    for (int a = 0; a < WT; a++) bsum[a] = asum[a] + __shfl_xor(asum[a], 32, 64);
    // (interleaved columns with WT = 4: the four column tiles of a lane are 16 contiguous bytes -- one ds_write_b128 / ds_read_b128 instead of
    // four 4-byte accesses at a 16-byte lane stride, which run four-way bank-conflicted)
    constexpr bool V4 = COLS_IL && CT == 4;
    if (wave == 0) {
        if constexpr (V4) {
#pragma unroll
            for (int a = 0; a < WT; a++)
#pragma unroll
                for (int r = 0; r < 16; r++)
                    *reinterpret_cast<float4*>(&ldsW[(WT * rho(r, h) + a) * LDL + WT * g]) = make_float4(acc[a][0][r], acc[a][1][r], acc[a][2][r], acc[a][3][r]);
        } else {
#pragma unroll
        for (int a = 0; a < WT; a++)
#pragma unroll
            for (int b = 0; b < CT; b++)
#pragma unroll
                for (int r = 0; r < 16; r++) ldsW[(WT * rho(r, h) + a) * LDL + (COLS_IL ? WT * g + b : 32 * b + g)] = acc[a][b][r];
        }
        if (h == 0) {
#pragma unroll
            for (int a = 0; a < WT; a++) ldsB[WT * g + a] = bsum[a];
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int turn = 1; turn < 4; turn++) {
        if (wave == turn) {
            if constexpr (V4) {
#pragma unroll
                for (int a = 0; a < WT; a++) {
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        float4* q = reinterpret_cast<float4*>(&ldsW[(WT * rho(r, h) + a) * LDL + WT * g]);
                        float4 v = *q;
                        v.x += acc[a][0][r]; v.y += acc[a][1][r]; v.z += acc[a][2][r]; v.w += acc[a][3][r];
                        *q = v;
                    }
                    __builtin_amdgcn_sched_barrier(0);   // 16 read-add-writes at a time (hoisted ds_reads would spill)
                }
            } else
#pragma unroll
            for (int a = 0; a < WT; a++)
#pragma unroll
                for (int b = 0; b < CT; b++) {
#pragma unroll
                    for (int r = 0; r < 16; r++) ldsW[(WT * rho(r, h) + a) * LDL + (COLS_IL ? WT * g + b : 32 * b + g)] += acc[a][b][r];
                    __builtin_amdgcn_sched_barrier(0);   // 16 read-add-writes at a time (256 hoisted ds_reads would spill)
                }
            if (h == 0) {
#pragma unroll
                for (int a = 0; a < WT; a++) ldsB[WT * g + a] += bsum[a];
            }
        }
        __syncthreads();
    }
}

template <int WT, bool ROWS>
__global__ void __launch_bounds__(256, 1) deform_wgrad_kernel(WgradArgs a) {
    // the accumulator rows are ldl floats wide: W for the head products, 32 * ceil(C*L / 32) <= 128 for the trunk product -- which is WIDER than
    // W at net_width 64 with C*L = 96 / 128 (W * W floats were too few there: rows past the array were dropped and the bias row overlapped)
    constexpr int W = WT * 32, LDM = W > 128 ? W : 128;
    __shared__ __attribute__((aligned(16))) float lds[W * LDM + W];
    // job of this workgroup
    int j = 0;
#pragma unroll
    for (int q = 1; q < FDGS_NUM_HEADS + 1; q++)
        if (q < a.njobs && (int)blockIdx.x >= a.job[q].first_block) j = q;
    const WgradJob J = a.job[j];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane & 31, h = lane >> 5;
    const int blk = (int)blockIdx.x - J.first_block;
    // this workgroup's share of the live tiles, split over its four waves
    const long long nlive = (long long)(int)as_const(a.counters)[ROWS ? 5 : 1];
    const const_u32p live_list = as_const(ROWS ? a.rows : a.live);
    const int t0 = (int)(nlive * blk / J.nblocks), t1 = (int)(nlive * (blk + 1) / J.nblocks);
    if (t1 <= t0) return;           // (uniform: nothing to add to the weight gradients)
    const int per = (t1 - t0 + 3) / 4;
    int wb = t0 + __builtin_amdgcn_readfirstlane(wave) * per, we = wb + per;      // (wave-uniform: the list is read with scalar loads)
    if (wb > t1) wb = t1;
    if (we > t1) we = t1;
    float* ldsW = lds;
    float* ldsB = lds + W * LDM;
    const int CTn = (J.ncols + 31) / 32;
    // (every wave joins, also one whose slice is empty: the reduction inside is a workgroup-wide protocol)
    if (J.ncols == W) wgrad_wave<WT, WT, true, 8, ROWS>(J, W, live_list, wb, we, ldsW, ldsB, g, h, wave);
    else if (CTn == 1) wgrad_wave<WT, 1, false, 16, ROWS>(J, W, live_list, wb, we, ldsW, ldsB, g, h, wave);
    else if (CTn == 2) wgrad_wave<WT, 2, false, 16, ROWS>(J, W, live_list, wb, we, ldsW, ldsB, g, h, wave);
    else if (CTn == 3) wgrad_wave<WT, 3, false, 8, ROWS>(J, W, live_list, wb, we, ldsW, ldsB, g, h, wave);
    else if constexpr (WT != 4) wgrad_wave<WT, 4, false, 8, ROWS>(J, W, live_list, wb, we, ldsW, ldsB, g, h, wave);   // (W = 128, 128 columns) is the interleaved case
    const int ldl = J.ncols == W ? W : 32 * CTn;
    for (int i = threadIdx.x; i < W * ldl; i += 256) {
        const int m = i / ldl, c = i - m * ldl;
        const float v = ldsW[i];
        if (c < J.ncols && v != 0.f) atomicAdd(&J.dW[(size_t)m * J.ldw + c], v);
    }
    if ((int)threadIdx.x < W && ldsB[threadIdx.x] != 0.f) atomicAdd(&J.db[threadIdx.x], ldsB[threadIdx.x]);
}
