// deform_layers.h -- what every deformation kernel shares: the MFMA wrappers, the HexPlane sampling helpers, DeformDev (the forward's kernel
// argument) and the dense-layer building blocks on the matrix cores.  Included first by deform.hip, inside namespace fdgs.

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
typedef float f32x4 __attribute__((ext_vector_type(4)));
// 16 independent 4x4x1 outer products: lane 4b+i holds A_b[i], lane 4b+j holds B_b[j], lane 4b+j register i gets D_b[i][j]
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 0);
}
// same with block ABID of the A operand broadcast to all 16 blocks (CBSZ = 4)
template <int ABID>
__device__ __forceinline__ f32x4 mfma4_bcast(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 4, ABID, 0);
}
__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; i++) z[i] = 0.f;
    return z;
}
// feature row held by (tile t, register r, half h) of the MFMA C/D layout
__device__ __forceinline__ int frow(int t, int r, int h) { return t * 32 + (r & 3) + 8 * (r >> 2) + 4 * h; }

// outputs per head (pos, scale, rot, opacity, shs) and the column of the head's outputs in the packed [N,64] gradient rows
__host__ __device__ __forceinline__ int head_k(int hd) { return hd == 0 ? 3 : hd == 1 ? 3 : hd == 2 ? 4 : hd == 3 ? 1 : 48; }
__host__ __device__ __forceinline__ int head_off(int hd) { return hd == 0 ? 0 : hd == 1 ? 3 : hd == 2 ? 6 : hd == 3 ? 10 : 16; }
constexpr int GCOLS = 64;
// first row of a head's k output rows in arrays that stack the five heads (3 + 3 + 4 + 1 + 48 = 59 rows)
__host__ __device__ __forceinline__ int head_row0(int hd) { return hd == 0 ? 0 : hd == 1 ? 3 : hd == 2 ? 6 : hd == 3 ? 10 : 11; }

// ------------------------------------------------------------------------------------------------ HexPlane gather
// AxisSample, axis_sample and query_coord -- the index arithmetic -- live in hexplane_ops.h (contraction off, shared with the host twin)
__host__ __device__ __forceinline__ void plane_axes(int k, int& a, int& b) {
    // pairs (0,1),(0,2),(0,3),(1,2),(1,3),(2,3): a indexes the plane's width, b its height
    a = k < 3 ? 0 : (k < 5 ? 1 : 2);
    b = k < 3 ? k + 1 : (k < 5 ? k - 1 : 3);
}

// inv2[i] = 2 / (aabb[3+i] - aabb[i]), the same float division the reference performs, done once on the host (three
// full-precision divisions per lane are ~36 VALU instructions)
struct AabbScale { float inv2[3]; };
static AabbScale aabb_scale(const fdgs_deform_params* p) {
    AabbScale s;
    for (int i = 0; i < 3; i++) s.inv2[i] = 2.0f / (p->aabb[3 + i] - p->aabb[i]);
    return s;
}
struct DeformDev {
    fdgs_deform_params p;
    fdgs_deform_out out;
    AabbScale sc;
    int F;
    int small_heads;   // 1: k <= 4 heads on the 4x4x1 MFMA (default), 0: padded 32x32x2 tiles (the host always passes 1)
    int split_tail;    // 1: the tiles left over after the last full round of the persistent loop are split by head over the waves (FDGS_D1_SPLIT)
    // optional saved activations for the backward (rows < Npad): features [Np][F], relu(hidden) [Np][W], relu(h1) [slot][Np][W]
    float *sv_feat, *sv_rh, *sv_h1;
    int ntiles;                     // 32-Gaussian tiles (a multiple of 4)
    unsigned long long* prof;       // development builds (-DFDGS_PROFILE_D1): cycle sums per phase
    uint32_t* sv_hmask;             // [Npad/32][64 lanes][4]: bit r of word t = relu(hidden) tile t register r > 0 (what D2's lane needs)
    int Npad;
    int head_slot[FDGS_NUM_HEADS];
    const float* packed;            // form 16: W0 / W1 as operand streams (pack_weights16_kernel)
    const float* feat;              // weight-stationary form: the HexPlane features [Npad][F] (deform_gather_kernel)
    unsigned head_mask;             // weight-stationary form: bit hd = head hd is on (a scalar the lanes can test with their own head index)
    int skew;                       // form 16: start delay (s_memtime ticks) of the second half of the grid (a constant set by fdgs_deform_fwd)
};

// 4 consecutive features f0..f0+3 (all inside one level because C % 8 == 0) of one Gaussian.
// Texel addresses are 32-bit byte offsets from the (wave-uniform) plane pointer: one VALU op per address and the
// SGPR-base + VGPR-offset load form, instead of 64-bit multiply-adds per corner (planes are < 2^32 bytes by validation).
// The level index is the same for both lane halves (C % 8 == 0): computed from the wave-uniform chunk index and pinned
// to an SGPR, so that the resolutions and plane pointers are scalar (kernarg) loads.  (Derived from the per-lane f0 they
// were two dependent VECTOR loads per chunk, each a full memory round trip in front of the 24 texel requests.)
__device__ __forceinline__ float4 gather_chunk(const fdgs_deform_params& p, int j, int h, const float* q) {
    const int lvl = __builtin_amdgcn_readfirstlane((8 * j) / p.C);
    const int c0 = 8 * j + 4 * h - lvl * p.C;
    float4 prod = make_float4(1.f, 1.f, 1.f, 1.f);
#pragma unroll
    for (int k = 0; k < 6; k++) {
        int a, b;
        plane_axes(k, a, b);
        const int Wd = p.res[lvl][a], Hd = p.res[lvl][b];
        const AxisSample sx = axis_sample(q[a], Wd), sy = axis_sample(q[b], Hd);
        const char* P = reinterpret_cast<const char*>(p.planes[lvl][k]);
        const uint32_t texel = (uint32_t)p.C * 4u, cb = (uint32_t)c0 * 4u;
        const uint32_t r0 = (uint32_t)(sy.i0 * Wd) * texel + cb, r1 = (uint32_t)(sy.i1 * Wd) * texel + cb;
        const uint32_t x0 = (uint32_t)sx.i0 * texel, x1 = (uint32_t)sx.i1 * texel;
        const float4 v00 = *reinterpret_cast<const float4*>(P + (r0 + x0));
        const float4 v01 = *reinterpret_cast<const float4*>(P + (r0 + x1));
        const float4 v10 = *reinterpret_cast<const float4*>(P + (r1 + x0));
        const float4 v11 = *reinterpret_cast<const float4*>(P + (r1 + x1));
        const float w00 = sx.w0 * sy.w0, w01 = sx.w1 * sy.w0, w10 = sx.w0 * sy.w1, w11 = sx.w1 * sy.w1;
        prod.x *= v00.x * w00 + v01.x * w01 + v10.x * w10 + v11.x * w11;
        prod.y *= v00.y * w00 + v01.y * w01 + v10.y * w10 + v11.y * w11;
        prod.z *= v00.z * w00 + v01.z * w01 + v10.z * w10 + v11.z * w11;
        prod.w *= v00.w * w00 + v01.w * w01 + v10.w * w10 + v11.w * w11;
    }
    return prod;
}

__device__ __forceinline__ void load_query(const fdgs_deform_params& p, const AabbScale& sc, int n, float* q, float* xyz) {
    xyz[0] = p.xyz[3 * (size_t)n]; xyz[1] = p.xyz[3 * (size_t)n + 1]; xyz[2] = p.xyz[3 * (size_t)n + 2];
#pragma unroll
    for (int i = 0; i < 3; i++) q[i] = query_coord(xyz[i], p.aabb[i], sc.inv2[i]);
    q[3] = p.time ? p.time[n] : p.time_scalar;
}

// Two adjacent chunks j0, j0+1 of ONE level (C >= 16: their channels are the two halves of the same 32 texel bytes): the
// four axis samples and the texel offsets are computed once and all 48 texel requests are issued before the first one is
// consumed -- one memory round trip for the pair.  (Chunk by chunk the four round trips of a 32-feature gather were 12 %
// of D1 in its in-kernel cycle profile.)  Same arithmetic per chunk as gather_chunk.
__device__ __forceinline__ void gather_chunk_pair(const fdgs_deform_params& p, int j0, int h, const float* q, float4& out0, float4& out1) {
    const int lvl = __builtin_amdgcn_readfirstlane((8 * j0) / p.C);
    const int c0 = 8 * j0 + 4 * h - lvl * p.C;
    AxisSample S[4];
#pragma unroll
    for (int ax = 0; ax < 4; ax++) S[ax] = axis_sample(q[ax], p.res[lvl][ax]);
    float4 v[6][4], u[6][4];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        int a, b;
        plane_axes(k, a, b);
        const int Wd = p.res[lvl][a];
        const AxisSample sx = S[a], sy = S[b];
        const char* P = reinterpret_cast<const char*>(p.planes[lvl][k]);
        const uint32_t texel = (uint32_t)p.C * 4u, cb = (uint32_t)c0 * 4u;
        const uint32_t r0 = (uint32_t)(sy.i0 * Wd) * texel + cb, r1 = (uint32_t)(sy.i1 * Wd) * texel + cb;
        const uint32_t x0 = (uint32_t)sx.i0 * texel, x1 = (uint32_t)sx.i1 * texel;
        v[k][0] = *reinterpret_cast<const float4*>(P + (r0 + x0)); u[k][0] = *reinterpret_cast<const float4*>(P + (r0 + x0 + 32u));
        v[k][1] = *reinterpret_cast<const float4*>(P + (r0 + x1)); u[k][1] = *reinterpret_cast<const float4*>(P + (r0 + x1 + 32u));
        v[k][2] = *reinterpret_cast<const float4*>(P + (r1 + x0)); u[k][2] = *reinterpret_cast<const float4*>(P + (r1 + x0 + 32u));
        v[k][3] = *reinterpret_cast<const float4*>(P + (r1 + x1)); u[k][3] = *reinterpret_cast<const float4*>(P + (r1 + x1 + 32u));
    }
    __builtin_amdgcn_sched_barrier(0);
    out0 = make_float4(1.f, 1.f, 1.f, 1.f); out1 = out0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        int a, b;
        plane_axes(k, a, b);
        const AxisSample sx = S[a], sy = S[b];
        const float w00 = sx.w0 * sy.w0, w01 = sx.w1 * sy.w0, w10 = sx.w0 * sy.w1, w11 = sx.w1 * sy.w1;
        out0.x *= v[k][0].x * w00 + v[k][1].x * w01 + v[k][2].x * w10 + v[k][3].x * w11;
        out0.y *= v[k][0].y * w00 + v[k][1].y * w01 + v[k][2].y * w10 + v[k][3].y * w11;
        out0.z *= v[k][0].z * w00 + v[k][1].z * w01 + v[k][2].z * w10 + v[k][3].z * w11;
        out0.w *= v[k][0].w * w00 + v[k][1].w * w01 + v[k][2].w * w10 + v[k][3].w * w11;
        out1.x *= u[k][0].x * w00 + u[k][1].x * w01 + u[k][2].x * w10 + u[k][3].x * w11;
        out1.y *= u[k][0].y * w00 + u[k][1].y * w01 + u[k][2].y * w10 + u[k][3].y * w11;
        out1.z *= u[k][0].z * w00 + u[k][1].z * w01 + u[k][2].z * w10 + u[k][3].z * w11;
        out1.w *= u[k][0].w * w00 + u[k][1].w * w01 + u[k][2].w * w10 + u[k][3].w * w11;
    }
}

// features of lane (g,h): chunk j holds features 8j+4h .. +3 = registers 4(j%4)..+3 of tile j/4
template <int FCH>
__device__ __forceinline__ void gather_features(const fdgs_deform_params& p, const float* q, int h, f32x16* feat) {
    auto put = [&](int j, const float4& v) {
        feat[j / 4][4 * (j % 4) + 0] = v.x; feat[j / 4][4 * (j % 4) + 1] = v.y;
        feat[j / 4][4 * (j % 4) + 2] = v.z; feat[j / 4][4 * (j % 4) + 3] = v.w;
    };
#pragma unroll
    for (int j = 0; j < FCH; j += 2) {
        if (j + 1 < FCH && (8 * j) / p.C == (8 * (j + 1)) / p.C) {   // (wave-uniform) both chunks in one level
            float4 v0, v1;
            gather_chunk_pair(p, j, h, q, v0, v1);
            put(j, v0); put(j + 1, v1);
        } else {
            put(j, gather_chunk(p, j, h, q));
            if (j + 1 < FCH) put(j + 1, gather_chunk(p, j + 1, h, q));
        }
    }
}

// ------------------------------------------------------------------------------------------------ MFMA layers
// Register layouts.  rho(r,h) = row of the 32x32 MFMA C/D tile that register r holds in lane half h.
//   * "chunk" layout (HexPlane features, F = 8*FCH): tile j/4, registers 4(j%4)..+3 of lane (g,h) hold features
//     8j+4h..+3 of Gaussian g  (== feature 32*tile + rho(r,h));
//   * "interleaved" layout (hidden activations, T = W/32 tiles): tile t, register r of lane (g,h) holds feature
//     T*rho(r,h) + t.  With it BOTH products read the torch-layout weights with one 16-byte load per lane:
//       Y = W X   : A-lane (row, h) needs W[row][T*rho(r,h) + t], t = 0..T-1  -> one vector load per r feeds T MFMAs;
//       dX = W^T dY: A-lane (i, h) needs W[f][T*i + xt],       xt = 0..T-1 -> one vector load per k-step feeds T MFMAs
//     (the transposed product with the naive 32t+row layout needs T separate dword loads per k-step).
// Every A operand is software-prefetched PD steps ahead (the compiler serialises load -> wait -> 4 MFMA otherwise:
// round-1 profile, 52 % / 31 % MFMA utilisation in D1 / D2).
__device__ __forceinline__ constexpr int rho(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

template <int VW>
struct AVec { float v[VW]; };
template <int VW>
__device__ __forceinline__ AVec<VW> ldv(const float* __restrict__ p) {
    AVec<VW> a;
    if constexpr (VW == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        a.v[0] = q.x; a.v[1] = q.y; a.v[2] = q.z; a.v[3] = q.w;
    } else if constexpr (VW == 2) {
        const float2 q = *reinterpret_cast<const float2*>(p);
        a.v[0] = q.x; a.v[1] = q.y;
    } else {
        a.v[0] = *p;
    }
    return a;
}

// Y[ot] = bias + W X, X in interleaved layout (KT tiles, K = 32*KT), W row-major [out_dim][ld].
// Output rows: ROW_IL ? interleaved (row = OT*i + ot) : standard (row = 32*ot + i), rows >= out_dim are duplicates
// of the last valid row (never read back).  Usage: setup(); preload(); ...; run().
template <int KT, int OT, bool ROW_IL, int PD, bool CLAMP = true>
struct DenseIL {
    const float* rp[OT];
    const float* bp[OT];
    float bv[OT];
    AVec<KT> buf[PD][OT];
    // The bias enters as one extra MFMA k-step (A = bias[row] in the k = 0 half, 0 in the k = 1 half; B = 1): its four
    // dword loads ride with the weight prefetch instead of stalling the first MFMA of the layer on 64 bias loads.
    __device__ __forceinline__ void setup(const float* __restrict__ Wm, const float* __restrict__ bias, int ld, int out_dim, int g, int h) {
#pragma unroll
        for (int ot = 0; ot < OT; ot++) {
            int row = ROW_IL ? OT * g + ot : 32 * ot + g;
            if (CLAMP) row = row < out_dim ? row : out_dim - 1;
            rp[ot] = Wm + (size_t)row * ld + KT * 4 * h;
            bp[ot] = bias + row;
        }
    }
    __device__ __forceinline__ void fetch(int s, AVec<KT>* dst) const {
#pragma unroll
        for (int ot = 0; ot < OT; ot++) dst[ot] = ldv<KT>(rp[ot] + KT * rho(s, 0));
    }
    __device__ __forceinline__ void preload() {
#pragma unroll
        for (int ot = 0; ot < OT; ot++) bv[ot] = *bp[ot];
#pragma unroll
        for (int s = 0; s < PD; s++) fetch(s, buf[s]);
    }
    // ---- k <= 4 output rows (position / scale / rotation / opacity heads): instead of padding the 3..4 rows to a 32-row
    // MFMA tile (64 MFMAs of 64 cycles at 9-12 % use) the product runs on v_mfma_f32_4x4x1_16b: block b = lane/4 holds
    // four Gaussians (B = the interleaved activation register as it is), A-lane 4b+i = W[i][feature of this half];
    // 64 instructions of 8 cycles.  The two lane halves hold partial sums over their halves of the features.
    __device__ __forceinline__ void setup4(const float* __restrict__ Wm, const float* __restrict__ bias, int ld, int out_dim, int g, int h) {
        static_assert(OT == 1, "small-output form has one output tile");
        int row = g & 3;
        row = row < out_dim ? row : out_dim - 1;
        rp[0] = Wm + (size_t)row * ld + KT * 4 * h;
        bp[0] = bias + row;
    }
    // returns out[i] (i < 4) of the lane's Gaussian in .x .y .z .w, valid in every lane
    __device__ __forceinline__ f32x4 run4(const f32x16* X) {
        f32x4 acc[KT];
#pragma unroll
        for (int t = 0; t < KT; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 16; s++) {
            const AVec<KT> cur = buf[s % PD][0];
            if (s + PD < 16) fetch(s + PD, buf[s % PD]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < KT; t++) acc[t] = mfma4(cur.v[t], X[t][s], acc[t]);
        }
        f32x4 sum = acc[0];
#pragma unroll
        for (int t = 1; t < KT; t++) sum += acc[t];
        // lane 4b+j register i = partial out[i] of Gaussian (4b+j)&31 over this half's features; bias of row i sits in the
        // lanes with (lane & 3) == i
        f32x4 out;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float tot = sum[i] + __shfl_xor(sum[i], 32, 64);
            out[i] = tot + __shfl(bv[0], i, 4);
        }
        return out;
    }
    struct NoHook { __device__ __forceinline__ void operator()(int) const {} };
    __device__ __forceinline__ void run(const f32x16* X, f32x16* Y, int h) { run(X, Y, h, NoHook()); }
    // `hook(s)` is issued once per k-walk step, in the shadow of that step's MFMAs (used to drain a staged tile)
    template <class Hook>
    __device__ __forceinline__ void run(const f32x16* X, f32x16* Y, int h, Hook hook) {
#pragma unroll
        for (int ot = 0; ot < OT; ot++) Y[ot] = mfma32(h == 0 ? bv[ot] : 0.f, 1.0f, zero16());
#pragma unroll
        for (int s = 0; s < 16; s++) {
            AVec<KT> cur[OT];
#pragma unroll
            for (int ot = 0; ot < OT; ot++) cur[ot] = buf[s % PD][ot];
            if (s + PD < 16) fetch(s + PD, buf[s % PD]);
            hook(s);
            __builtin_amdgcn_sched_barrier(0);   // keep the prefetch PD steps ahead (the scheduler sinks it to its use otherwise)
#pragma unroll
            for (int t = 0; t < KT; t++)
#pragma unroll
                for (int ot = 0; ot < OT; ot++) Y[ot] = mfma32(cur[ot].v[t], X[t][s], Y[ot]);
        }
    }
};

// hid[ot] = b0 + W0 feat: feat in chunk layout (FCH chunks of 8 features), output rows interleaved (row = OT*i + ot)
template <int FCH, int OT, int PD>
struct DenseTrunk {
    const float* rp[OT];
    const float* bp;
    float bv[OT];
    float4 buf[PD][OT];
    __device__ __forceinline__ void setup(const float* __restrict__ Wm, const float* __restrict__ bias, int ld, int g, int h) {
#pragma unroll
        for (int ot = 0; ot < OT; ot++) rp[ot] = Wm + (size_t)(OT * g + ot) * ld + 4 * h;
        bp = bias + OT * g;
    }
    __device__ __forceinline__ void fetch(int j, float4* dst) const {
#pragma unroll
        for (int ot = 0; ot < OT; ot++) dst[ot] = *reinterpret_cast<const float4*>(rp[ot] + 8 * j);
    }
    __device__ __forceinline__ void preload() {
#pragma unroll
        for (int ot = 0; ot < OT; ot++) bv[ot] = bp[ot];
#pragma unroll
        for (int s = 0; s < PD; s++) if (s < FCH) fetch(s, buf[s]);
    }
    __device__ __forceinline__ void run(const f32x16* feat, f32x16* Y, int h) {
#pragma unroll
        for (int ot = 0; ot < OT; ot++) Y[ot] = mfma32(h == 0 ? bv[ot] : 0.f, 1.0f, zero16());
#pragma unroll
        for (int j = 0; j < FCH; j++) {
            float4 cur[OT];
#pragma unroll
            for (int ot = 0; ot < OT; ot++) cur[ot] = buf[j % PD][ot];
            if (j + PD < FCH) fetch(j + PD, buf[j % PD]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ot = 0; ot < OT; ot++) Y[ot] = mfma32(cur[ot].x, feat[j / 4][4 * (j % 4) + 0], Y[ot]);
#pragma unroll
            for (int ot = 0; ot < OT; ot++) Y[ot] = mfma32(cur[ot].y, feat[j / 4][4 * (j % 4) + 1], Y[ot]);
#pragma unroll
            for (int ot = 0; ot < OT; ot++) Y[ot] = mfma32(cur[ot].z, feat[j / 4][4 * (j % 4) + 2], Y[ot]);
#pragma unroll
            for (int ot = 0; ot < OT; ot++) Y[ot] = mfma32(cur[ot].w, feat[j / 4][4 * (j % 4) + 3], Y[ot]);
        }
    }
};

// dX[xt] += W^T dY: dY interleaved (YT tiles, feature f = YT*rho(r,h) + t), W row-major [32*YT][ld].
// COL_IL: dX interleaved with XT tiles (column XT*i + xt, one vector load per k-step);
// else:   dX in tile layout (column 32*xt + i, clamped to in_valid-1; rows beyond are never read back).
template <int YT, int XT, bool COL_IL, int PD>
struct DenseT {
    static constexpr int VW = COL_IL ? XT : 1;
    static constexpr int NL = COL_IL ? 1 : XT;   // loads per k-step
    const float* cp[NL];
    int ld;
    AVec<VW> buf[PD][NL];
    __device__ __forceinline__ void setup(const float* __restrict__ Wm, int ld_, int in_valid, int g, int h) {
        ld = ld_;
#pragma unroll
        for (int x = 0; x < NL; x++) {
            int col = COL_IL ? XT * g : 32 * x + g;
            col = col < in_valid ? col : in_valid - 1;
            cp[x] = Wm + (size_t)(YT * 4 * h) * ld_ + col;
        }
    }
    // k-step s = (r, t): r = s / YT, t = s % YT  ->  weight row YT*rho(r,0) + t (+ YT*4*h folded into cp)
    __device__ __forceinline__ void fetch(int s, AVec<VW>* dst) const {
        const int r = s / YT, t = s % YT;
#pragma unroll
        for (int x = 0; x < NL; x++) dst[x] = ldv<VW>(cp[x] + (size_t)(YT * rho(r, 0) + t) * ld);
    }
    __device__ __forceinline__ void preload() {
#pragma unroll
        for (int s = 0; s < PD; s++) fetch(s, buf[s]);
    }
    __device__ __forceinline__ void run(const f32x16* dY, f32x16* dX) {
#pragma unroll
        for (int s = 0; s < 16 * YT; s++) {
            AVec<VW> cur[NL];
#pragma unroll
            for (int x = 0; x < NL; x++) cur[x] = buf[s % PD][x];
            if (s + PD < 16 * YT) fetch(s + PD, buf[s % PD]);
            __builtin_amdgcn_sched_barrier(0);
            const float b = dY[s % YT][s / YT];
#pragma unroll
            for (int xt = 0; xt < XT; xt++) dX[xt] = mfma32(COL_IL ? cur[0].v[xt] : cur[xt].v[0], b, dX[xt]);
        }
    }
};

template <int T>
__device__ __forceinline__ void relu_inplace(f32x16* x) {
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) x[t][r] = fmaxf(x[t][r], 0.f);
}

// interleaved activations -> row-major [n][W] global rows: register r of the T tiles = T consecutive features
template <int T>
__device__ __forceinline__ void store_il(float* __restrict__ rowp, const f32x16* x, int h) {
#pragma unroll
    for (int r = 0; r < 16; r++) {
        if constexpr (T == 4) *reinterpret_cast<float4*>(rowp + 4 * rho(r, h)) = make_float4(x[0][r], x[1][r], x[2][r], x[3][r]);
        else *reinterpret_cast<float2*>(rowp + 2 * rho(r, h)) = make_float2(x[0][r], x[1][r]);
    }
}

// [32 gaussians][W] tile of interleaved activations -> 32 contiguous global rows, through a padded per-wave LDS tile:
// the lanes park "their" Gaussian's row (store_il layout), then the wave copies the 32*W floats out lane-consecutively
// (1 KB per store instruction).  Direct store_il to global writes 16-byte pieces at 512-byte strides: measured +0.19 ms on
// the forward for the 960 MB of saved activations.
template <int T>
__device__ __forceinline__ void store_tile_coalesced(float* lds_tile, float* __restrict__ gdst, const f32x16* x, int g, int h, int lane) {
    constexpr int W = 32 * T, STRIDE = W + 4;
    __builtin_amdgcn_wave_barrier();
    store_il<T>(lds_tile + g * STRIDE, x, h);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < T * 4; j++) {
        const int e4 = j * 64 + lane, row = e4 / (W / 4), c4 = e4 - row * (W / 4);
        reinterpret_cast<float4*>(gdst)[e4] = *reinterpret_cast<const float4*>(lds_tile + row * STRIDE + 4 * c4);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + __expf(-x)); }

__device__ __forceinline__ int next_head(const int* head_on, int hd) {
    hd++;
    while (hd < FDGS_NUM_HEADS && !head_on[hd]) hd++;
    return hd;
}

__device__ __forceinline__ int next_head_m(unsigned mask, int hd) {
    hd++;
    while (hd < FDGS_NUM_HEADS && !((mask >> hd) & 1u)) hd++;
    return hd;
}
