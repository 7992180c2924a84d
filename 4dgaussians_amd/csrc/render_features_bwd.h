// render_features_bwd.h -- the adjoint of the feature pass with respect to its values (included by render.hip, inside namespace fdgs,
// behind render_features_kernel: it uses that unit's replay walk, blend_replay.h, and FEAT_CH).
//
//     dvalues[row, c] += sum over the frame's pixels of w(row, pixel) * G[c, pixel],      G = dL/dfeatures
//
// A replay walk that stages the ids, one workgroup per tile and chunk of FEAT_CH = 16 channels (blockIdx.y) as render_features_kernel's.
// What differs is where w goes.  Per tile and chunk the work is a small GEMM, dV[entry, c] = sum over the 256 pixels of
// w[entry, pixel] * G[c, pixel], and the contraction over the pixels runs on the matrix cores:
//
//   * a wave owns 64 pixels (four lines of the tile).  Its operand G -- 64 pixels x 16 channels -- is loaded ONCE per tile and chunk, one
//     coalesced load per channel with the lane's own pixel, scaled on the way for a normalised forward (G / A, IEEE division, where
//     A > min_alpha, else 0; A is the alpha image the forward wrote), zero for a pixel outside the image or a channel >= C;
//   * the wave walks its list in blocks of 16 entries and keeps w of ITS pixel for the 16 in registers (0 where the entry is skipped or
//     lies behind the lane's own end);
//   * both operands are 16 x 64 matrices held as [k][lane = pixel]; v_mfma_f32_16x16x4_f32 wants one float per lane, A[l & 15][l >> 4] and
//     B[l >> 4][l & 15], so the wave transposes through a private LDS park (park_transpose: register s of lane l becomes element
//     [l & 15][pixel s + 16 (l >> 4)]; rows 65 floats apart, so neither the writes nor the reads meet in a bank) -- G once, w per block;
//   * 16 MFMAs (k = 4 pixels each) leave dV[entry 4 (l >> 4) + r][channel l & 15] in register r of lane l.  The instruction is exact
//     float32 (no reduced-precision inputs).  A block in which no lane of the wave has w > 0 is skipped (one ballot);
//   * the four waves' partial [16][16] results meet in LDS as the contribution pass's do -- plain stores into per-wave slots, one word
//     per wave that says whether it wrote (no clearing) --, block by block: the slot is the first 1 KB of the wave's own park, free
//     again once the transposed w is in registers.  After a barrier the workgroup adds the slots in wave order and issues at most ONE
//     float atomic per (tile, entry, channel): 16 neighbouring lanes own the 16 channels of one entry, so one instruction covers whole
//     64-byte rows where the caller's rows are aligned.  A zero sum issues no atomic; a row outside [0, rows) -- a -1 of the map
//     included -- is dropped.  A second barrier hands the parks back.  (Two barriers per 16 entries cost less than the LDS that
//     collecting 32 or 64 entries per flush takes: 25.9 KB and six workgroups per CU against 34.3 / 42.5 KB and four / three, the
//     kernel 0.19 against 0.22 / 0.24 ms on config 4 at C = 16)
//
// Nothing of the frame is written.  The gradient is with respect to `values` only: for a normalised forward the path through A is
// geometry, which a bake does not have.
// NON-FINITE GRADIENT IMAGES ARE OUT OF CONTRACT: the contraction multiplies every w of a block, zeros included, with every G of the
// wave's pixels, so one inf or NaN in G reaches (as 0 * inf = NaN) the other entries of that wave's block, not only its own contributors.
#pragma once

constexpr int FBWD_PARK = 65;                // floats from one row of a wave's park to the next
static_assert(FEAT_CH == 16, "render_features_bwd_kernel: one 16x16x4 MFMA tile of channels per workgroup");

typedef float fbwd_f32x4 __attribute__((ext_vector_type(4)));

struct FeatBwdArgs : ReplayArgs {
    int C; const float* grad;                // dL/dfeatures [C,H,W]
    const float* alpha; float min_alpha;     // min_alpha >= 0: the forward divided by A = alpha[pixel] where A > min_alpha
    const int32_t* row_map; int rows;        // opt [P]: the row of `dvalues` Gaussian g is accumulated into
    float* dvalues; int dvalue_stride;
};

// v[k] of lane p = M[k][p], a 16 x 64 matrix  ->  v[s] of lane l = M[l & 15][s + 16 * (l >> 4)]: the operand of MFMA step s (lane l holds
// row l & 15 of the matrix at the step's pixel k = l >> 4).  `park`: the wave's own 16 * FBWD_PARK floats of LDS.
__device__ __forceinline__ void park_transpose(float* park, int lane, float (&v)[16]) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < 16; k++) park[k * FBWD_PARK + lane] = v[k];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    const float* src = park + (lane & 15) * FBWD_PARK + 16 * (lane >> 4);
#pragma unroll
    for (int s = 0; s < 16; s++) v[s] = src[s];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

__global__ void __launch_bounds__(256) render_features_bwd_kernel(FeatBwdArgs a) {
#pragma clang fp contract(off)
    const ReplayPixel px = replay_pixel<false>(a);
    if (px.tile < 0) return;
    __shared__ float4 sA[256], sB[256];
    __shared__ uint32_t sG[256];
    __shared__ float sPark[4][16 * FBWD_PARK];
    __shared__ uint32_t sHit[4];                         // per wave: it left a result for this block
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    float* const park = sPark[wv];
    const int c0 = (int)blockIdx.y * FEAT_CH;                                // this chunk's first channel
    const int nch = a.C - c0 < FEAT_CH ? a.C - c0 : FEAT_CH;                 // ... and how many of its sixteen exist (>= 1: the grid)
    const bool inside = px.inside;
    const size_t pix = px.pix, hw = (size_t)a.H * a.W;
    const ReplayLengths len = replay_lengths<false>(a, px.tile, px.own);
    if (len.rounds == 0) return;                                             // (uniform: nothing was blended into this tile)
    const int wave_mine = replay_wave_mine(len.mine);
    uint32_t g_cur = replay_gid(a, len, 0), g_nxt = len.rounds > 1 ? replay_gid(a, len, 1) : 0u;
    float4 rA = a.recA[g_cur], rB = a.recB[g_cur];
    // the wave's operand G: channel k of the lane's own pixel, then transposed once
    float gop[16];
    {
        float scale = 1.0f;
        bool live = inside;
        if (a.min_alpha >= 0.0f && inside) {
            scale = a.alpha[pix];
            live = scale > a.min_alpha;                                      // (a NaN A: false, as the forward's test)
        }
#pragma unroll
        for (int k = 0; k < 16; k++) {
            float g = 0.0f;
            if (live && k < nch) {
                g = a.grad[(size_t)(c0 + k) * hw + pix];
                if (a.min_alpha >= 0.0f) g = g / scale;                      // (IEEE division, the forward's F / A)
            }
            gop[k] = g;
        }
        park_transpose(park, lane, gop);
    }
    float T = 1.0f;
    int seen = 0;                            // entries of the list this lane has passed
    for (int r = 0; r < len.rounds; r++) {
        if (__syncthreads_count(seen >= len.mine) == 256) break;
        const int left = len.todo - r * 256;
        const int staged = left < 256 ? left : 256;                         // entries of this round
        sA[t] = rA; sB[t] = rB; sG[t] = g_cur;
        __syncthreads();
        if (r + 1 < len.rounds) { g_cur = g_nxt; rA = a.recA[g_cur]; rB = a.recB[g_cur]; }
        if (r + 2 < len.rounds) g_nxt = replay_gid(a, len, r + 2);
        const int rem = len.mine - seen;
        const int wave_rem = wave_mine - seen;
        const int lim = wave_rem < staged ? wave_rem : staged;              // where this wave's walk of the round ends
        for (int j0 = 0; j0 < staged; j0 += 16) {                           // (uniform over the workgroup)
            bool wrote = false;
            if (j0 < lim) {                                                  // (uniform over the wave)
                float w16[16];
                bool any = false;
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const int j = j0 + k;                                    // (< 256: sA / sB hold a record for every j, a copy of the list's last behind its end)
                    float w = 0.0f;
                    if (j < rem) {
                        const ReplayWeight e = replay_weight(sA[j], sB[j], px.pxf, px.pyf, T);
                        w = e.w;
                        T = e.T;
                    }
                    w16[k] = w;
                    any = any || w > 0.0f;
                }
                if (__ballot(any) != 0ull) {                                 // (uniform over the wave)
                    park_transpose(park, lane, w16);
                    // (two accumulators, even and odd steps: a dependent MFMA of this shape issues every 40 cycles, an independent one every 32)
                    fbwd_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int s = 0; s < 16; s += 2) {
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w16[s], gop[s], acc, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w16[s + 1], gop[s + 1], acc1, 0, 0, 0);
                    }
                    acc = acc + acc1;
                    // register r of lane l: entry 4 (l >> 4) + r of the block, channel l & 15, left at word 64 r + l of the wave's park
                    // (free again: park_transpose ends behind its reads) -- lane-consecutive words, no two lanes of a store on one bank
                    park[lane] = acc[0]; park[64 + lane] = acc[1]; park[128 + lane] = acc[2]; park[192 + lane] = acc[3];
                    wrote = true;
                }
            }
            if (lane == 0) sHit[wv] = wrote ? 1u : 0u;
            __syncthreads();
            const uint32_t h0 = sHit[0], h1 = sHit[1], h2 = sHit[2], h3 = sHit[3];
            if ((h0 | h1) | (h2 | h3)) {                                     // (uniform over the workgroup)
                // thread t takes word t of the four slots: entry 4 ((t >> 4) & 3) + (t >> 6), channel t & 15 -- 16 neighbouring lanes own
                // the 16 channels of one entry
                const int ch = t & 15, jj = j0 + 4 * ((t >> 4) & 3) + (t >> 6);
                float s = 0.0f;
                if (h0) s = s + sPark[0][t];
                if (h1) s = s + sPark[1][t];
                if (h2) s = s + sPark[2][t];
                if (h3) s = s + sPark[3][t];
                if (jj < staged && ch < nch && s != 0.0f) {
                    const int32_t row = replay_row(a, sG[jj], a.row_map, (uint32_t)a.rows);
                    if (row >= 0) atomicAdd(a.dvalues + (size_t)row * (size_t)a.dvalue_stride + (size_t)(c0 + ch), s);
                }
            }
            __syncthreads();                                                 // (the next block's transpose rewrites the parks, its end sHit)
        }
        seen += 256;
    }
}
