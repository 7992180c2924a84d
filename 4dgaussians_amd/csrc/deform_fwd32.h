// deform_fwd32.h -- D1 in its 32-GAUSSIAN form (deform_fwd_kernel: one wave owns 32 Gaussians on v_mfma_f32_32x32x2_f32).  Included by
// deform.hip inside namespace fdgs, after deform_layers.h.

// ------------------------------------------------------------------------------------------------ D1 forward
#ifndef FDGS_D1_PD1
#define FDGS_D1_PD1 2
#endif
template <int WT>
struct FwdPD { static constexpr int L1 = WT == 4 ? 2 : 4, L2 = 8; };

template <int WT, int FCH>
__global__ void __launch_bounds__(256, 1) deform_fwd_kernel(DeformDev d) {
    constexpr int PD1 = WT == 4 ? FDGS_D1_PD1 : FwdPD<WT>::L1, PD2 = FwdPD<WT>::L2;
    const fdgs_deform_params& p = d.p;
    const bool tunable_small = d.small_heads != 0;
    // LDS: the four waves' staging tiles of the saved activations + the second-layer weights of all heads (59 rows, padded row
    // stride: rows i = 0..3 of a 4x4x1 product and the two lane halves fall into distinct banks).  The second layers are short
    // products (64 MFMAs of 8 cycles for a k <= 4 head) whose operand ring cannot cover an L2 round trip: read from LDS they lose
    // the ~2 k cycles per head that the in-kernel cycle profile charged to "L2" beyond its MFMA time.
    constexpr int LDW = WT * 32 + 4;
    __shared__ __attribute__((aligned(16))) float fwd_lds[4 * 32 * LDW + 59 * LDW];
    float* my_tile = fwd_lds + (threadIdx.x >> 6) * 32 * LDW;
    float* w2lds = fwd_lds + 4 * 32 * LDW;
    for (int hd_ = 0; hd_ < FDGS_NUM_HEADS; hd_++) {
        if (!p.head_on[hd_]) continue;
        const int k_ = head_k(hd_), r0_ = head_row0(hd_);
        for (int i = threadIdx.x; i < k_ * (WT * 8); i += 256) {
            const int r = i / (WT * 8), c4 = i - r * (WT * 8);
            *reinterpret_cast<float4*>(w2lds + (r0_ + r) * LDW + 4 * c4) = reinterpret_cast<const float4*>(p.w2[hd_])[i];
        }
    }
    __syncthreads();
    constexpr int FT = (FCH + 3) / 4;
    const int lane = threadIdx.x & 63, g0 = lane & 31, h0 = lane >> 5;
    // Every wave walks its own tiles (32 Gaussians each): nothing in the body synchronises the workgroup, so with
    // gridDim.x = #CUs the kernel is persistent -- no workgroup relaunch between tiles and no SIMD waiting for the slowest
    // of the four waves of its workgroup; with gridDim.x = ntiles / 4 the loop runs once (FDGS_D1_WGS selects).
#ifdef FDGS_PROFILE_D1
    unsigned long long pacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long pt = __builtin_amdgcn_s_memtime();
#define D1_TICK(ph) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); pacc[ph] += t_ - pt; pt = t_; } while (0)
#else
#define D1_TICK(ph) do { } while (0)
#endif
    // Persistent loop: wave w takes tiles w, w + #waves, ...  The tiles left over after the last FULL round would keep a few waves busy
    // for a whole tile while the others idle (300 k Gaussians: 9 376 tiles on 1 024 waves = 9 full rounds + 160 tiles, 8.4 % of the
    // kernel).  Where they fit, those tiles are split BY HEAD instead: wave u takes head u % nh of tile u / nh -- every such wave repeats
    // the gather and the trunk (cheap) and evaluates one head, so the last round lasts about a third of a tile.  The first wave of a tile
    // ("primary") also writes what is per tile rather than per head: saved features / trunk activations, outputs of switched-off heads.
    unsigned all_heads = 0u;
    int nh = 0;
#pragma unroll
    for (int i = 0; i < FDGS_NUM_HEADS; i++) if (p.head_on[i]) { all_heads |= 1u << i; nh++; }
    const int nwaves = (int)gridDim.x * 4, wave_id = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const int full_rounds = d.ntiles / nwaves, rem = d.ntiles - full_rounds * nwaves;
    const bool split = d.split_tail != 0 && nh > 1 && rem > 0 && rem * nh <= nwaves;
    for (int it = 0; it <= full_rounds; it++) {
    int tile = it * nwaves + wave_id;
    unsigned head_mask = all_heads;
    bool primary = true;
    if (it == full_rounds) {
        if (split) {
            if (wave_id >= rem * nh) break;
            tile = full_rounds * nwaves + wave_id / nh;
            int ord = wave_id % nh, hsel = -1;
            for (int i = 0; i < FDGS_NUM_HEADS; i++) if (p.head_on[i] && ord-- == 0) hsel = i;
            head_mask = 1u << hsel;
            primary = wave_id % nh == 0;
        } else if (tile >= d.ntiles) {
            break;
        }
    }
    int g = g0, h = h0;
    asm volatile("" : "+v"(g), "+v"(h));   // keeps the per-layer weight addresses from being hoisted out of the tile loop
    const size_t tile_n0 = (size_t)tile * 32;       // first Gaussian slot of this wave's tile
    const int n_raw = tile * 32 + g;
    const bool live = n_raw < p.N;
    const int n = live ? n_raw : p.N - 1;
    const int W = WT * 32;
    DenseTrunk<FCH, WT, 2> T0;
    T0.setup(p.w0, p.b0, d.F, g, h);
    T0.preload();
    int hd = next_head_m(head_mask, -1);
    DenseIL<WT, WT, true, PD1, false> L1;
    if (hd < FDGS_NUM_HEADS) { L1.setup(p.w1[hd], p.b1[hd], W, W, g, h); L1.preload(); }
    float q[4], xyz[3];
    load_query(p, d.sc, n, q, xyz);
    // every per-Gaussian input of the epilogues is fetched now (one HBM round trip under the gather) instead of once per
    // head behind its last MFMA
    float in_sc[3], in_op, in_sh[24];
#pragma unroll
    for (int i = 0; i < 3; i++) in_sc[i] = p.scales[3 * (size_t)n + i];
    const float4 in_rot = reinterpret_cast<const float4*>(p.rotations)[n];
    in_op = p.opacity[n];
#pragma unroll
    for (int u = 0; u < 6; u++) {
        const int row0 = (u < 4 ? 0 : 32) + 8 * (u & 3) + 4 * h;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int m = row0 + i;
            in_sh[4 * u + i] = m < 3 ? p.shs_dc[(size_t)p.shs_dc_stride * n + m] : p.shs_rest[(size_t)p.shs_rest_stride * n + (m - 3)];
        }
    }
    f32x16 feat[FT];
#pragma unroll
    for (int t = 0; t < FT; t++) feat[t] = zero16();
    D1_TICK(0);
    gather_features<FCH>(p, q, h, feat);
    D1_TICK(1);
    const size_t n_row = (size_t)n_raw;   // saved rows are indexed by the un-clamped Gaussian slot (< Npad)
    if (d.sv_feat && primary) {
#pragma unroll
        for (int j = 0; j < FCH; j++)
            *reinterpret_cast<float4*>(d.sv_feat + n_row * d.F + 8 * j + 4 * h) =
                make_float4(feat[j / 4][4 * (j % 4)], feat[j / 4][4 * (j % 4) + 1], feat[j / 4][4 * (j % 4) + 2], feat[j / 4][4 * (j % 4) + 3]);
    }
    f32x16 hid[WT];
    T0.run(feat, hid, h);
    relu_inplace<WT>(hid);  // every consumer of the trunk output starts with ReLU (scene/deformation.py:61-65)
    // saved activations leave through the LDS tile: parked right after they are computed, copied out (lane-consecutive,
    // 1 KB per store) one 1-KB piece per k-walk step of the NEXT hidden layer, i.e. in the shadow of its MFMAs
    float* pending_dst = nullptr;
    constexpr int TSTRIDE = WT * 32 + 4;
    auto park = [&](const f32x16* x, float* dst) {
        store_il<WT>(my_tile + g * TSTRIDE, x, h);
        pending_dst = dst;
    };
    auto drain_piece = [&](int j) {     // pieces j = 0 .. 4*WT-1 of 64 float4 each
        if (pending_dst && j < WT * 4) {
            const int e4 = j * 64 + lane, row = e4 / (W / 4), c4 = e4 - row * (W / 4);
            reinterpret_cast<float4*>(pending_dst)[e4] = *reinterpret_cast<const float4*>(my_tile + row * TSTRIDE + 4 * c4);
        }
    };
    if (d.sv_rh && primary) park(hid, d.sv_rh + tile_n0 * W);
    if (d.sv_hmask && primary) {   // the backward's ReLU mask of the trunk output, in its own lane layout: one 16-byte load there
        uint32_t m[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int t = 0; t < WT; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) m[t] |= (hid[t][r] > 0.f ? 1u : 0u) << r;
        reinterpret_cast<uint4*>(d.sv_hmask)[(size_t)(tile_n0 / 32) * 64 + lane] = make_uint4(m[0], m[1], m[2], m[3]);
    }

    const bool writer = live && h == 0;
    // epilogue of head hd applied to the head's output delta (zero for a switched-off head: it returns its input
    // unchanged, scene/deformation.py:106-146)
    auto epilogue = [&](int hd_, const f32x16& o0, const f32x16& o1) {
        if (hd_ == FDGS_HEAD_POS) {
            if (writer) {
                d.out.xyz[3 * (size_t)n] = xyz[0] + o0[0]; d.out.xyz[3 * (size_t)n + 1] = xyz[1] + o0[1];
                d.out.xyz[3 * (size_t)n + 2] = xyz[2] + o0[2];
            }
        } else if (hd_ == FDGS_HEAD_SCALE) {
            if (writer) {
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const float v = in_sc[i] + o0[i];
                    d.out.scales[3 * (size_t)n + i] = p.activate ? __expf(v) : v;
                }
            }
        } else if (hd_ == FDGS_HEAD_ROT) {
            if (writer) {
                float v0 = in_rot.x + o0[0], v1 = in_rot.y + o0[1], v2 = in_rot.z + o0[2], v3 = in_rot.w + o0[3];
                if (p.activate) {
                    const float nrm = sqrtf(v0 * v0 + v1 * v1 + v2 * v2 + v3 * v3);
                    const float inv = 1.0f / fmaxf(nrm, 1e-12f);  // F.normalize eps (scene/gaussian_model.py:44)
                    v0 *= inv; v1 *= inv; v2 *= inv; v3 *= inv;
                    if (d.out.rot_norm) d.out.rot_norm[n] = nrm;
                }
                reinterpret_cast<float4*>(d.out.rotations)[n] = make_float4(v0, v1, v2, v3);
            }
        } else if (hd_ == FDGS_HEAD_OPACITY) {
            if (writer) {
                const float v = in_op + o0[0];
                d.out.opacity[n] = p.activate ? sigmoidf_(v) : v;
            }
        } else {
            // shs [N,16,3] = cat(features_dc, features_rest) (+ delta): rows 8u+4h..+3 of tile 0 (u<4) and tile 1 (u<2)
            if (live) {
#pragma unroll
                for (int u = 0; u < 6; u++) {
                    const int row0 = (u < 4 ? 0 : 32) + 8 * (u & 3) + 4 * h;
                    float v[4];
#pragma unroll
                    for (int i = 0; i < 4; i++) v[i] = in_sh[4 * u + i] + (u < 4 ? o0[4 * (u & 3) + i] : o1[4 * (u & 3) + i]);
                    *reinterpret_cast<float4*>(d.out.shs + 48 * (size_t)n + row0) = make_float4(v[0], v[1], v[2], v[3]);
                }
            }
        }
    };
    {
        const f32x16 z = zero16();
        for (int h0 = 0; h0 < FDGS_NUM_HEADS; h0++)
            if (!p.head_on[h0] && primary) epilogue(h0, z, z);
    }

    D1_TICK(2);
    while (hd < FDGS_NUM_HEADS) {
        const int k = head_k(hd);
        DenseIL<WT, 1, false, PD2> L2, L2b;
        const bool small = k <= 4 && tunable_small;
        const float* w2h = w2lds + head_row0(hd) * LDW;
        if (small) L2.setup4(w2h, p.b2[hd], LDW, k, g, h);
        else L2.setup(w2h, p.b2[hd], LDW, k < 32 ? k : 32, g, h);
        L2.preload();
        f32x16 h1[WT];
        L1.run(hid, h1, h, drain_piece);
        D1_TICK(3);
        relu_inplace<WT>(h1);
        if (d.sv_h1) park(h1, d.sv_h1 + ((size_t)d.head_slot[hd] * d.Npad + tile_n0) * W);
        if (k > 32) { L2b.setup(w2h + 32 * LDW, p.b2[hd] + 32, LDW, k - 32, g, h); L2b.preload(); }
        const int nxt = next_head_m(head_mask, hd);
        if (nxt < FDGS_NUM_HEADS) { L1.setup(p.w1[nxt], p.b1[nxt], W, W, g, h); L1.preload(); }
        f32x16 o0 = zero16(), o1 = zero16();
        D1_TICK(4);
        if (small) {
            const f32x4 o4 = L2.run4(h1);
            o0[0] = o4[0]; o0[1] = o4[1]; o0[2] = o4[2]; o0[3] = o4[3];
        } else {
            L2.run(h1, &o0, h);
        }
        if (k > 32) L2b.run(h1, &o1, h);
        D1_TICK(5);
        epilogue(hd, o0, o1);
        D1_TICK(6);
        hd = nxt;
    }
    // the last parked tile has no following layer to hide under
#pragma unroll
    for (int j = 0; j < WT * 4; j++) drain_piece(j);
    D1_TICK(7);
    }   // tile loop
#ifdef FDGS_PROFILE_D1
    if (d.prof && lane == 0) {
        for (int i = 0; i < 8; i++) atomicAdd(&d.prof[i], pacc[i]);
        atomicAdd(&d.prof[8], 1ull);
    }
#endif
}
