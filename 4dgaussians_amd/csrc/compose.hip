// compose.hip -- scene composition: one baked state (or the blend of two) moved by a placement into its rows of a composite state.
//
// One memory-bound streaming kernel; the arithmetic is the host/device functions of compose_ops.h that fdgs_state_place_host calls as
// well, compiled without contraction: the device result is the host result bit for bit, whichever lane computes a value.
//
// The SH stream is 192 of the 236 bytes of a row, so it decides the cost.  A lane that walked its own 192-byte row would touch 64
// separate lines per wave instruction; instead a workgroup (256 threads) takes a TILE of 64 rows:
//   load   the tile's 64 x 48 floats are contiguous and 16-byte aligned in the source: consecutive lanes load consecutive float4 pieces
//          (of a and, when blending, of b), blend them and write them to LDS.  A piece never straddles two rows (48 = 12 * 4).
//   mix    LDS row stride 49 floats: in the band mix lane = row, wave = colour channel (waves 0 .. 2), so the 32 lanes of a half wave
//          read 32 different banks.  Each lane reads the 16 coefficients of its channel, applies place_sh and writes them back in place.
//          The band matrices are kernel arguments, i.e. wave-uniform scalars.  Meanwhile wave 3 does the small fields, one row per lane.
//   store  the destination has 4-byte alignment only (a model's first row is anywhere in the composite): up to three single floats to
//          the first 16-byte boundary, consecutive lanes on consecutive float4 pieces from there, up to three single floats at the end.
// Without the SH stream in field_mask there is no LDS stage and a workgroup takes 256 rows, one per lane.
// No atomics; every load and store is guarded by row < N.
//
// fdgs_state_place_rows is the same kernel for a model baked sparsely: the sources are COMPACT [D, width] arrays and row r goes to row
// rows[r] of the model's N rows in the composite.  The load and the mix are the ones above (the compact SH rows of a tile are contiguous);
// the 64 indices of a tile are read once into LDS (-1 past the end of the list) and every access through one is guarded by one unsigned
// compare against N.  A row's 192 bytes land at out.shs + 48 * rows[r]; 192 is a multiple of 16, so every row has the alignment of
// out.shs and the host decides the store ONCE per launch: float4 pieces, 12 consecutive lanes per row, or single floats, 48 per row.
#include "common.h"
#include "compose_ops.h"

namespace fdgs {

constexpr int PLACE_TILE = 64;                  // rows per workgroup when the SH stream is selected
constexpr int SH_FLOATS = 48;
constexpr int SH_LDS_STRIDE = SH_FLOATS + 1;    // odd: lane = row reads hit 32 distinct banks per half wave
constexpr unsigned PLACE_ALL_FIELDS = 31u;

struct PlaceArgs {
    fdgs_placement p;
    fdgs_state_arrays a, b, out;
    int N, blend;
    unsigned mask;
    float w;
};

__device__ __forceinline__ void place_small_fields(const PlaceArgs& g, long long row) {
    const float w = g.w;
    if (g.mask & 1u) {
        const float* a = g.a.xyz + 3 * row;
        float o[3];
        place_row_xyz(g.p, a, g.blend ? g.b.xyz + 3 * row : nullptr, w, o);
        float* out = g.out.xyz + 3 * row;
        out[0] = o[0]; out[1] = o[1]; out[2] = o[2];
    }
    if (g.mask & 2u) {
        const float* a = g.a.scales + 3 * row;
        float o[3];
        place_row_scales(g.p, a, g.blend ? g.b.scales + 3 * row : nullptr, w, o);
        float* out = g.out.scales + 3 * row;
        out[0] = o[0]; out[1] = o[1]; out[2] = o[2];
    }
    if (g.mask & 4u) {
        const float4 va = reinterpret_cast<const float4*>(g.a.rotations)[row];
        const float qa[4] = {va.x, va.y, va.z, va.w};
        float v[4] = {va.x, va.y, va.z, va.w}, o[4];
        if (g.blend) {
            const float4 vb = reinterpret_cast<const float4*>(g.b.rotations)[row];
            const float qb[4] = {vb.x, vb.y, vb.z, vb.w};
            blend_quat(qa, qb, w, v);
        }
        place_rotation(g.p, v, o);
        float* out = g.out.rotations + 4 * row;
        out[0] = o[0]; out[1] = o[1]; out[2] = o[2]; out[3] = o[3];
    }
    if (g.mask & 8u) g.out.opacity[row] = place_row_opacity(g.a.opacity + row, g.blend ? g.b.opacity + row : nullptr, w);
}

__global__ void __launch_bounds__(256) state_place_kernel(const PlaceArgs g) {
    const int tid = threadIdx.x;
    if (!(g.mask & 16u)) {                                                   // (uniform) small fields only: 256 rows per workgroup
        const long long row = (long long)blockIdx.x * 256 + tid;
        if (row < g.N) place_small_fields(g, row);
        return;
    }
    __shared__ float tile[PLACE_TILE * SH_LDS_STRIDE];
    const long long r0 = (long long)blockIdx.x * PLACE_TILE;
    const int rows = g.N - r0 < PLACE_TILE ? (int)(g.N - r0) : PLACE_TILE;   // >= 1: the grid is cdiv(N, 64)
    const int nfl = rows * SH_FLOATS;                                        // floats of this tile, a multiple of 4
    // ---- load (+ blend): piece q = floats [4 q, 4 q + 4) of the tile, inside row q / 12
    {
        const float4* __restrict__ a4 = reinterpret_cast<const float4*>(g.a.shs + r0 * SH_FLOATS);
        const float4* __restrict__ b4 = g.blend ? reinterpret_cast<const float4*>(g.b.shs + r0 * SH_FLOATS) : nullptr;
        for (int q = tid; 4 * q < nfl; q += 256) {
            float4 v = a4[q];
            if (g.blend) {
                const float4 u = b4[q];
                v = make_float4(blend_lerp(v.x, u.x, g.w), blend_lerp(v.y, u.y, g.w), blend_lerp(v.z, u.z, g.w), blend_lerp(v.w, u.w, g.w));
            }
            float* t = tile + 4 * q + q / 12;                                // row * 49 + column, row = q / 12
            t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
        }
    }
    __syncthreads();
    // ---- mix: waves 0 .. 2 = colour channel, lane = row; wave 3 = the small fields of the tile's rows
    if (tid < 192) {
        const int row = tid & 63, ch = tid >> 6;
        if (row < rows) {
            float* t = tile + row * SH_LDS_STRIDE + ch;
            float in[16], o[16];
#pragma unroll
            for (int j = 0; j < 16; j++) in[j] = t[3 * j];
            place_sh(g.p, in, o, 1);
#pragma unroll
            for (int j = 0; j < 16; j++) t[3 * j] = o[j];
        }
    } else if (g.mask & 15u) {
        const int row = tid - 192;
        if (row < rows) place_small_fields(g, r0 + row);
    }
    __syncthreads();
    // ---- store: float f of the tile is tile[f + f / 48]
    float* __restrict__ dst = g.out.shs + r0 * SH_FLOATS;
    const int head_raw = (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3u)) & 3u);   // floats to the 16-byte boundary
    const int head = head_raw < nfl ? head_raw : nfl;
    const int nq = (nfl - head) >> 2, tail0 = head + 4 * nq;
    for (int q = tid; q < nq; q += 256) {
        const int f = head + 4 * q;
        float4 v;
        v.x = tile[f + f / SH_FLOATS];
        v.y = tile[f + 1 + (f + 1) / SH_FLOATS];
        v.z = tile[f + 2 + (f + 2) / SH_FLOATS];
        v.w = tile[f + 3 + (f + 3) / SH_FLOATS];
        *reinterpret_cast<float4*>(dst + f) = v;
    }
    if (tid < head) dst[tid] = tile[tid + tid / SH_FLOATS];
    if (tid >= 64 && tid - 64 < nfl - tail0) {                               // (another wave than the head's)
        const int f = tail0 + tid - 64;
        dst[f] = tile[f + f / SH_FLOATS];
    }
}


// ---- fdgs_state_place_rows.  The first two phases of a tile are state_place_kernel's: `rows` (>= 1) contiguous source rows from r0 on.
// They are written again here, and state_place_kernel is left as it was: calling these functions from it changed the code generated for
// it (27 more instructions, 50 more waits), and that kernel is every dense composite's frame.  The arithmetic is shared either way.
// load (+ blend): piece q = floats [4 q, 4 q + 4) of the tile, inside row q / 12
__device__ __forceinline__ void load_sh_tile(const PlaceArgs& g, long long r0, int rows, float* tile) {
    const int nfl = rows * SH_FLOATS;                                        // floats of this tile, a multiple of 4
    const float4* __restrict__ a4 = reinterpret_cast<const float4*>(g.a.shs + r0 * SH_FLOATS);
    const float4* __restrict__ b4 = g.blend ? reinterpret_cast<const float4*>(g.b.shs + r0 * SH_FLOATS) : nullptr;
    for (int q = threadIdx.x; 4 * q < nfl; q += 256) {
        float4 v = a4[q];
        if (g.blend) {
            const float4 u = b4[q];
            v = make_float4(blend_lerp(v.x, u.x, g.w), blend_lerp(v.y, u.y, g.w), blend_lerp(v.z, u.z, g.w), blend_lerp(v.w, u.w, g.w));
        }
        float* t = tile + 4 * q + q / 12;                                    // row * 49 + column, row = q / 12
        t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
    }
}

// mix, waves 0 .. 2: wave = colour channel, lane = row
__device__ __forceinline__ void mix_sh_tile(const PlaceArgs& g, int rows, float* tile) {
    const int row = threadIdx.x & 63, ch = threadIdx.x >> 6;
    if (row < rows) {
        float* t = tile + row * SH_LDS_STRIDE + ch;
        float in[16], o[16];
#pragma unroll
        for (int j = 0; j < 16; j++) in[j] = t[3 * j];
        place_sh(g.p, in, o, 1);
#pragma unroll
        for (int j = 0; j < 16; j++) t[3 * j] = o[j];
    }
}

// place_small_fields with the source and the destination row apart: row `src` of a (and b) -> row `dst` of out
__device__ __forceinline__ void place_small_fields_to(const PlaceArgs& g, long long src, long long dst) {
    const float w = g.w;
    if (g.mask & 1u) {
        const float* a = g.a.xyz + 3 * src;
        float o[3];
        place_row_xyz(g.p, a, g.blend ? g.b.xyz + 3 * src : nullptr, w, o);
        float* out = g.out.xyz + 3 * dst;
        out[0] = o[0]; out[1] = o[1]; out[2] = o[2];
    }
    if (g.mask & 2u) {
        const float* a = g.a.scales + 3 * src;
        float o[3];
        place_row_scales(g.p, a, g.blend ? g.b.scales + 3 * src : nullptr, w, o);
        float* out = g.out.scales + 3 * dst;
        out[0] = o[0]; out[1] = o[1]; out[2] = o[2];
    }
    if (g.mask & 4u) {
        const float4 va = reinterpret_cast<const float4*>(g.a.rotations)[src];
        const float qa[4] = {va.x, va.y, va.z, va.w};
        float v[4] = {va.x, va.y, va.z, va.w}, o[4];
        if (g.blend) {
            const float4 vb = reinterpret_cast<const float4*>(g.b.rotations)[src];
            const float qb[4] = {vb.x, vb.y, vb.z, vb.w};
            blend_quat(qa, qb, w, v);
        }
        place_rotation(g.p, v, o);
        float* out = g.out.rotations + 4 * dst;
        out[0] = o[0]; out[1] = o[1]; out[2] = o[2]; out[3] = o[3];
    }
    if (g.mask & 8u) g.out.opacity[dst] = place_row_opacity(g.a.opacity + src, g.blend ? g.b.opacity + src : nullptr, w);
}


struct PlaceRowsArgs {
    PlaceArgs g;                                // a, b: compact [D, width]; out: row 0 of the model's N rows; N bounds the indices
    const int32_t* rows;
    int D, vec;                                 // vec: out.shs is 16-byte aligned, and with it every row of it
};

__global__ void __launch_bounds__(256) state_place_rows_kernel(const PlaceRowsArgs h) {
    const PlaceArgs& g = h.g;
    const int tid = threadIdx.x;
    const unsigned N = (unsigned)g.N;
    if (!(g.mask & 16u)) {                                                   // (uniform) small fields only: one listed row per lane
        const long long r = (long long)blockIdx.x * 256 + tid;
        if (r < h.D) {
            const unsigned row = (unsigned)h.rows[r];
            if (row < N) place_small_fields_to(g, r, row);
        }
        return;
    }
    __shared__ float tile[PLACE_TILE * SH_LDS_STRIDE];
    __shared__ int rows_s[PLACE_TILE];
    const long long r0 = (long long)blockIdx.x * PLACE_TILE;
    const int rows = h.D - r0 < PLACE_TILE ? (int)(h.D - r0) : PLACE_TILE;   // >= 1: the grid is cdiv(D, 64)
    if (tid < PLACE_TILE) rows_s[tid] = tid < rows ? h.rows[r0 + tid] : -1;
    load_sh_tile(g, r0, rows, tile);
    __syncthreads();
    if (tid < 192) {
        mix_sh_tile(g, rows, tile);
    } else if (g.mask & 15u) {
        const unsigned row = (unsigned)rows_s[tid - 192];
        if (row < N) place_small_fields_to(g, r0 + (tid - 192), row);
    }
    __syncthreads();
    // ---- store: row lr of the tile to row rows_s[lr] of out; a slot past the end of the list holds -1 and fails the compare too
    if (h.vec) {
        float4* __restrict__ o4 = reinterpret_cast<float4*>(g.out.shs);
#pragma unroll
        for (int q = tid; q < PLACE_TILE * (SH_FLOATS / 4); q += 256) {
            const int lr = q / (SH_FLOATS / 4), piece = q - lr * (SH_FLOATS / 4);
            const unsigned row = (unsigned)rows_s[lr];
            if (row >= N) continue;
            const float* t = tile + lr * SH_LDS_STRIDE + 4 * piece;
            o4[(size_t)row * (SH_FLOATS / 4) + piece] = make_float4(t[0], t[1], t[2], t[3]);
        }
    } else {
        float* __restrict__ o = g.out.shs;
#pragma unroll 4
        for (int f = tid; f < PLACE_TILE * SH_FLOATS; f += 256) {
            const int lr = f / SH_FLOATS, c = f - lr * SH_FLOATS;
            const unsigned row = (unsigned)rows_s[lr];
            if (row >= N) continue;
            o[(size_t)row * SH_FLOATS + c] = tile[lr * SH_LDS_STRIDE + c];
        }
    }
}


static int check_place(const fdgs_placement* p, int N, unsigned field_mask, const fdgs_state_arrays* a, const fdgs_state_arrays* b, float w,
                       const fdgs_state_arrays* out, bool device) {
    FDGS_REQUIRE(N >= 0, "bad N (negative)");
    FDGS_REQUIRE(field_mask <= PLACE_ALL_FIELDS, "bad field_mask (bits 0 .. 4: positions, scales, rotations, opacity, SH)");
    FDGS_REQUIRE(p, "NULL pointer (placement)");
    FDGS_REQUIRE(p->mode == FDGS_PLACE_POINTS || p->mode == FDGS_PLACE_RIGID, "bad mode (FDGS_PLACE_POINTS | FDGS_PLACE_RIGID)");
    FDGS_REQUIRE(p->sh_degree >= 0 && p->sh_degree <= 3, "bad sh_degree (0 .. 3)");
    FDGS_REQUIRE(p->scale > 0.f && p->scale <= 3.402823466e38f, "bad scale (positive and finite)");
    FDGS_REQUIRE(w >= 0.f && w <= 1.f, "bad w (0 .. 1)");
    FDGS_REQUIRE(b || w == 0.f, "bad w (0 without a second state)");
    if (N == 0 || field_mask == 0) return FDGS_OK;
    FDGS_REQUIRE(a && out, "NULL pointer (a and out)");
    const float* pa[5] = {a->xyz, a->scales, a->rotations, a->opacity, a->shs};
    const float* po[5] = {out->xyz, out->scales, out->rotations, out->opacity, out->shs};
    const float* pb[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    if (b) { pb[0] = b->xyz; pb[1] = b->scales; pb[2] = b->rotations; pb[3] = b->opacity; pb[4] = b->shs; }
    for (int h = 0; h < 5; h++) {
        if (!(field_mask >> h & 1u)) continue;
        FDGS_REQUIRE(pa[h] && po[h] && (!b || pb[h]), "NULL pointer (a selected field needs a, out and, when blending, b)");
        if (device) {
            FDGS_REQUIRE(aligned_to(po[h], 4) && aligned_to(pa[h], 4) && (!b || aligned_to(pb[h], 4)), "arrays must be 4-byte aligned");
            if (h == 2 || h == 4)
                FDGS_REQUIRE(aligned_to(pa[h], 16) && (!b || aligned_to(pb[h], 16)), "the rotations and SH of a and b must be 16-byte aligned");
        }
    }
    return FDGS_OK;
}

// the rules of fdgs_state_place and of fdgs_state_scatter together; the selected fields and the placement do not depend on the row count, so
// check_place sees the D rows there are to read
static int check_place_rows(const fdgs_placement* p, int D, const int32_t* rows, int N, unsigned field_mask, const fdgs_state_arrays* a,
                            const fdgs_state_arrays* b, float w, const fdgs_state_arrays* out, bool device) {
    FDGS_REQUIRE(D >= 0 && N >= 0, "bad D or N (negative)");
    FDGS_REQUIRE(D <= N, "bad D (more listed rows than rows)");
    const int rc = check_place(p, D, field_mask, a, b, w, out, device);
    if (rc != FDGS_OK || D == 0 || field_mask == 0) return rc;
    FDGS_REQUIRE(rows, "NULL pointer (rows)");
    if (device) FDGS_REQUIRE(aligned_to(rows, 4), "rows must be 4-byte aligned");
    return FDGS_OK;
}

// host twin only, where the list is readable: the rule of the sparse playback entry points
static int check_row_list(int D, const int32_t* rows, int N) {
    for (int r = 0; r < D; r++) {
        FDGS_REQUIRE(rows[r] >= 0 && rows[r] < N, "bad rows (an entry outside [0, N))");
        FDGS_REQUIRE(r == 0 || rows[r] > rows[r - 1], "bad rows (not strictly ascending)");
    }
    return FDGS_OK;
}

// what fdgs_state_place_host does to one row: row `src` of a (and b) -> row `dst` of out
static void place_row_host(const fdgs_placement* p, unsigned field_mask, const fdgs_state_arrays* a, const fdgs_state_arrays* b, float w,
                           const fdgs_state_arrays* out, size_t src, size_t dst) {
    if (field_mask & 1u) place_row_xyz(*p, a->xyz + 3 * src, b ? b->xyz + 3 * src : nullptr, w, out->xyz + 3 * dst);
    if (field_mask & 2u) place_row_scales(*p, a->scales + 3 * src, b ? b->scales + 3 * src : nullptr, w, out->scales + 3 * dst);
    if (field_mask & 4u) place_row_rotation(*p, a->rotations + 4 * src, b ? b->rotations + 4 * src : nullptr, w, out->rotations + 4 * dst);
    if (field_mask & 8u) out->opacity[dst] = place_row_opacity(a->opacity + src, b ? b->opacity + src : nullptr, w);
    if (field_mask & 16u) {
        float v[SH_FLOATS];
        for (int k = 0; k < SH_FLOATS; k++) v[k] = b ? blend_lerp(a->shs[SH_FLOATS * src + k], b->shs[SH_FLOATS * src + k], w) : a->shs[SH_FLOATS * src + k];
        for (int ch = 0; ch < 3; ch++) place_sh(*p, v + ch, out->shs + SH_FLOATS * dst + ch, 3);
    }
}
}  // namespace fdgs

using namespace fdgs;

extern "C" int fdgs_state_place(void* stream_, const fdgs_placement* p, int N, unsigned field_mask, const fdgs_state_arrays* a,
                                const fdgs_state_arrays* b, float w, const fdgs_state_arrays* out) {
    const int rc = check_place(p, N, field_mask, a, b, w, out, true);
    if (rc != FDGS_OK || N == 0 || field_mask == 0) return rc;
    PlaceArgs g{};
    g.p = *p; g.a = *a; g.out = *out;
    if (b) g.b = *b;
    g.N = N; g.blend = b ? 1 : 0; g.mask = field_mask; g.w = w;
    const int blocks = cdiv(N, (field_mask & 16u) ? PLACE_TILE : 256);
    hipStream_t stream = (hipStream_t)stream_;
    { FDGS_TIMED("state_place", stream); hipLaunchKernelGGL(state_place_kernel, dim3(blocks), dim3(256), 0, stream, g); }
    FDGS_LAUNCH_CHECK("state_place", 0, stream);
    return FDGS_OK;
}

extern "C" int fdgs_state_place_host(const fdgs_placement* p, int N, unsigned field_mask, const fdgs_state_arrays* a,
                                     const fdgs_state_arrays* b, float w, const fdgs_state_arrays* out) {
    const int rc = check_place(p, N, field_mask, a, b, w, out, false);
    if (rc != FDGS_OK || N == 0 || field_mask == 0) return rc;
    for (size_t n = 0; n < (size_t)N; n++) place_row_host(p, field_mask, a, b, w, out, n, n);
    return FDGS_OK;
}

extern "C" int fdgs_state_place_rows(void* stream_, const fdgs_placement* p, int D, const int32_t* rows, int N, unsigned field_mask,
                                     const fdgs_state_arrays* a, const fdgs_state_arrays* b, float w, const fdgs_state_arrays* out) {
    const int rc = check_place_rows(p, D, rows, N, field_mask, a, b, w, out, true);
    if (rc != FDGS_OK || D == 0 || field_mask == 0) return rc;              // (N == 0 is D == 0)
    PlaceRowsArgs h{};
    h.g.p = *p; h.g.a = *a; h.g.out = *out;
    if (b) h.g.b = *b;
    h.g.N = N; h.g.blend = b ? 1 : 0; h.g.mask = field_mask; h.g.w = w;
    h.rows = rows; h.D = D; h.vec = aligned_to(out->shs, 16) ? 1 : 0;
    const int blocks = cdiv(D, (field_mask & 16u) ? PLACE_TILE : 256);
    hipStream_t stream = (hipStream_t)stream_;
    { FDGS_TIMED("state_place_rows", stream); hipLaunchKernelGGL(state_place_rows_kernel, dim3(blocks), dim3(256), 0, stream, h); }
    FDGS_LAUNCH_CHECK("state_place_rows", 0, stream);
    return FDGS_OK;
}

extern "C" int fdgs_state_place_rows_host(const fdgs_placement* p, int D, const int32_t* rows, int N, unsigned field_mask,
                                          const fdgs_state_arrays* a, const fdgs_state_arrays* b, float w, const fdgs_state_arrays* out) {
    int rc = check_place_rows(p, D, rows, N, field_mask, a, b, w, out, false);
    if (rc != FDGS_OK || D == 0 || field_mask == 0) return rc;
    if ((rc = check_row_list(D, rows, N)) != FDGS_OK) return rc;
    for (size_t r = 0; r < (size_t)D; r++) place_row_host(p, field_mask, a, b, w, out, r, (size_t)rows[r]);
    return FDGS_OK;
}
