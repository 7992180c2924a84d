// playback.hip -- what playing a trained model back needs beside the rasterizer: the temporal blend of two baked (deformed, activated)
// states, the vertex table of a per-timestamp 3DGS PLY, and the 8-bit image a frame is written or shown as.
//
// Three memory-bound streaming kernels (no LDS, no atomics); the arithmetic of each is ONE host/device function of playback_ops.h that the
// *_host entry points below call as well, compiled without contraction: the device result is the host result bit for bit.
//
//   fdgs_state_blend    one launch for every stream of the state: a lane moves 16 bytes (one float4 of a flat stream, or one quaternion);
//                       the n_floats % 4 floats at the end of a flat stream are one lane's scalar loop.
//   fdgs_pack_ply_rows  one thread per output float, consecutive threads write consecutive floats.
//   fdgs_image_rgb8     one thread per four pixels: three float4 loads (one per colour plane) and three dword stores when the planes and the
//                       output are aligned for them, scalar loads / byte stores otherwise and for the last H * W % 4 pixels.
//
// Sparse playback (a baked sequence that stores per timestamp only the rows that move) adds three more of the same kind:
//   fdgs_state_gather   compact[r] = full[rows[r]]   } 64 listed rows per workgroup, their indices held in 256 bytes of LDS; the SH stream
//   fdgs_state_scatter  out[rows[r]] = a[r] | blend  } as float4 pieces, 12 consecutive lanes per row; every indexed access guarded
//   fdgs_state_extent   per row and field the running maximum of |cur - ref|: four lanes per row, two shuffles, no LDS
#include "common.h"
#include "playback_ops.h"

namespace fdgs {

constexpr int BLEND_SEGMENTS = FDGS_MAX_BLEND_STREAMS + 1;      // the flat streams, then the rotations

struct BlendArgs {
    const float* a[BLEND_SEGMENTS];
    const float* b[BLEND_SEGMENTS];
    float* out[BLEND_SEGMENTS];
    unsigned long long n[BLEND_SEGMENTS];       // floats of a flat stream / quaternions of the rotation segment
    int first_block[BLEND_SEGMENTS + 1];        // workgroups [first_block[s], first_block[s + 1]) belong to segment s
    int nseg, rot_seg;                          // rot_seg = index of the rotation segment, -1 without one
    float w;
};

__global__ void __launch_bounds__(256) state_blend_kernel(const BlendArgs g) {
    int seg = 0;
    while (seg + 1 < g.nseg && (int)blockIdx.x >= g.first_block[seg + 1]) seg++;          // (uniform per workgroup)
    const unsigned long long i = (unsigned long long)((int)blockIdx.x - g.first_block[seg]) * 256 + threadIdx.x;
    const float* __restrict__ a = g.a[seg];
    const float* __restrict__ b = g.b[seg];
    float* __restrict__ out = g.out[seg];
    const unsigned long long n = g.n[seg];
    const float w = g.w;
    if (seg == g.rot_seg) {
        if (i >= n) return;
        const float4 va = reinterpret_cast<const float4*>(a)[i], vb = reinterpret_cast<const float4*>(b)[i];
        const float qa[4] = {va.x, va.y, va.z, va.w}, qb[4] = {vb.x, vb.y, vb.z, vb.w};
        float q[4];
        blend_quat(qa, qb, w, q);
        reinterpret_cast<float4*>(out)[i] = make_float4(q[0], q[1], q[2], q[3]);
        return;
    }
    const unsigned long long nq = n >> 2;
    if (i < nq) {
        const float4 va = reinterpret_cast<const float4*>(a)[i], vb = reinterpret_cast<const float4*>(b)[i];
        reinterpret_cast<float4*>(out)[i] = make_float4(blend_lerp(va.x, vb.x, w), blend_lerp(va.y, vb.y, w), blend_lerp(va.z, vb.z, w),
                                                        blend_lerp(va.w, vb.w, w));
    } else if (i == nq) {
        for (unsigned long long k = nq << 2; k < n; k++) out[k] = blend_lerp(a[k], b[k], w);
    }
}

__global__ void __launch_bounds__(256) pack_ply_rows_kernel(long long total, const float* __restrict__ xyz, const float* __restrict__ scales,
                                                            const float* __restrict__ rotations, const float* __restrict__ opacity,
                                                            const float* __restrict__ shs, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long n = i / PLY_COLUMNS;
    int array;
    const long long s = ply_source(n, (int)(i - n * PLY_COLUMNS), &array);
    const float* src = array == 0 ? xyz : array == 1 ? scales : array == 2 ? rotations : array == 3 ? opacity : shs;
    out[i] = array < 0 ? 0.f : src[s];
}

__global__ void __launch_bounds__(256) image_rgb8_kernel(long long HW, int mode, int vec_in, int vec_out, const float* __restrict__ image,
                                                         uint8_t* __restrict__ out) {
    const long long p0 = 4 * ((long long)blockIdx.x * 256 + threadIdx.x);
    if (p0 >= HW) return;
    const int cnt = HW - p0 < 4 ? (int)(HW - p0) : 4;
    float v[3][4] = {};
    if (vec_in && cnt == 4) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float4 t = *reinterpret_cast<const float4*>(image + c * HW + p0);
            v[c][0] = t.x; v[c][1] = t.y; v[c][2] = t.z; v[c][3] = t.w;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < cnt) v[c][k] = image[c * HW + p0 + k];
    }
    uint32_t px[12];
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int c = 0; c < 3; c++) px[3 * k + c] = rgb8_value(v[c][k], mode);
    uint8_t* o = out + 3 * p0;
    if (vec_out && cnt == 4) {
        uint32_t* o32 = reinterpret_cast<uint32_t*>(o);       // 3 * p0 = 12 bytes per lane: dword aligned when `out` is
#pragma unroll
        for (int j = 0; j < 3; j++) o32[j] = px[4 * j] | (px[4 * j + 1] << 8) | (px[4 * j + 2] << 16) | (px[4 * j + 3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 12; j++)
            if (j < 3 * cnt) o[j] = (uint8_t)px[j];
    }
}

// ---- sparse playback: rows picked by a list.  A workgroup takes 64 LISTED rows; their indices are read once into LDS (a slot past the
// end of the list holds -1), and every access through an index is guarded by one unsigned compare against N, which the -1 fails too.
constexpr int ROWS_TILE = 64;
constexpr int SH_PIECES = 12;                   // float4 pieces of an SH row (192 bytes, 16-byte aligned on both sides)
constexpr unsigned STATE_ALL_FIELDS = 31u;

struct RowsArgs {
    fdgs_state_arrays a, b, out;                // gather: a = full, out = compact; scatter: a (b) = compact, out = full
    const int32_t* rows;
    int D, N, blend;
    unsigned mask;
    float w;
};

// SCATTER: out[rows[r]] = a[r] (or the blend of a[r] and b[r]); else out[r] = a[rows[r]].  On the listed side consecutive lanes move
// consecutive float4 pieces of the SH stream (64 rows = 768 contiguous pieces), on the indexed side 12 consecutive lanes cover one row.
template <bool SCATTER>
__device__ __forceinline__ void move_listed_rows(const RowsArgs& g, int* rows_s) {
    const int tid = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * ROWS_TILE;
    if (tid < ROWS_TILE) rows_s[tid] = r0 + tid < g.D ? g.rows[r0 + tid] : -1;
    __syncthreads();
    const unsigned N = (unsigned)g.N;
    const bool blend = SCATTER && g.blend;
    const float w = g.w;
    if (g.mask & 16u) {
        const float4* __restrict__ a4 = reinterpret_cast<const float4*>(g.a.shs);
        const float4* __restrict__ b4 = reinterpret_cast<const float4*>(g.b.shs);
        float4* __restrict__ o4 = reinterpret_cast<float4*>(g.out.shs);
#pragma unroll
        for (int q = tid; q < ROWS_TILE * SH_PIECES; q += 256) {
            const int lr = q / SH_PIECES, piece = q - lr * SH_PIECES;
            const unsigned row = (unsigned)rows_s[lr];
            if (row >= N) continue;
            const size_t listed = (size_t)(r0 + lr) * SH_PIECES + piece, indexed = (size_t)row * SH_PIECES + piece;
            const size_t src = SCATTER ? listed : indexed, dst = SCATTER ? indexed : listed;
            float4 v = a4[src];
            if (blend) {
                const float4 u = b4[src];
                v = make_float4(blend_lerp(v.x, u.x, w), blend_lerp(v.y, u.y, w), blend_lerp(v.z, u.z, w), blend_lerp(v.w, u.w, w));
            }
            o4[dst] = v;
        }
    }
    if ((g.mask & 4u) && tid < ROWS_TILE) {                                   // wave 0: one quaternion per lane
        const unsigned row = (unsigned)rows_s[tid];
        if (row < N) {
            const size_t listed = (size_t)(r0 + tid), indexed = row;
            const size_t src = SCATTER ? listed : indexed, dst = SCATTER ? indexed : listed;
            float4 v = reinterpret_cast<const float4*>(g.a.rotations)[src];
            if (blend) {
                const float4 u = reinterpret_cast<const float4*>(g.b.rotations)[src];
                const float qa[4] = {v.x, v.y, v.z, v.w}, qb[4] = {u.x, u.y, u.z, u.w};
                float q[4];
                blend_quat(qa, qb, w, q);
                v = make_float4(q[0], q[1], q[2], q[3]);
            }
            reinterpret_cast<float4*>(g.out.rotations)[dst] = v;
        }
    }
#pragma unroll
    for (int h = 0; h < 2; h++) {                                             // positions: lanes 0 .. 191, scales: lanes 64 .. 255
        const int t = tid - ROWS_TILE * h;
        if (!(g.mask >> h & 1u) || t < 0 || t >= 3 * ROWS_TILE) continue;
        const int lr = t / 3, c = t - 3 * lr;
        const unsigned row = (unsigned)rows_s[lr];
        if (row >= N) continue;
        const size_t listed = (size_t)(r0 + lr) * 3 + c, indexed = (size_t)row * 3 + c;
        const size_t src = SCATTER ? listed : indexed, dst = SCATTER ? indexed : listed;
        const float* __restrict__ a = h ? g.a.scales : g.a.xyz;
        const float* __restrict__ b = h ? g.b.scales : g.b.xyz;
        float* __restrict__ out = h ? g.out.scales : g.out.xyz;
        out[dst] = blend ? blend_lerp(a[src], b[src], w) : a[src];
    }
    if ((g.mask & 8u) && tid >= 3 * ROWS_TILE) {                              // opacity: wave 3
        const int lr = tid - 3 * ROWS_TILE;
        const unsigned row = (unsigned)rows_s[lr];
        if (row < N) {
            const size_t listed = (size_t)(r0 + lr), indexed = row;
            const size_t src = SCATTER ? listed : indexed, dst = SCATTER ? indexed : listed;
            g.out.opacity[dst] = blend ? blend_lerp(g.a.opacity[src], g.b.opacity[src], w) : g.a.opacity[src];
        }
    }
}

__global__ void __launch_bounds__(256) state_gather_kernel(const RowsArgs g) {
    __shared__ int rows_s[ROWS_TILE];
    move_listed_rows<false>(g, rows_s);
}

__global__ void __launch_bounds__(256) state_scatter_kernel(const RowsArgs g) {
    __shared__ int rows_s[ROWS_TILE];
    move_listed_rows<true>(g, rows_s);
}

struct ExtentArgs {
    fdgs_state_arrays ref, cur;
    float* extent;
    int N;
    unsigned mask;
};

// four lanes per row, 64 rows per workgroup.  SH: lane `sub` of a row takes pieces sub, 4 + sub, 8 + sub, so the four lanes of a row read 64
// contiguous bytes per load and a wave 16 such runs; the four partial maxima meet in two shuffles.  Small fields: one field per lane.
__global__ void __launch_bounds__(256) state_extent_kernel(const ExtentArgs g) {
    const long long n = (long long)blockIdx.x * ROWS_TILE + (threadIdx.x >> 2);
    const int sub = threadIdx.x & 3;
    const bool live = n < g.N;
    if (g.mask & 16u) {                                                       // (uniform: every lane reaches the shuffles)
        float m = 0.f;
        if (live) {
            const float4* __restrict__ c4 = reinterpret_cast<const float4*>(g.cur.shs) + n * SH_PIECES;
            const float4* __restrict__ r4 = reinterpret_cast<const float4*>(g.ref.shs) + n * SH_PIECES;
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const float4 c = c4[4 * j + sub], r = r4[4 * j + sub];
                m = extent_step(m, c.x, r.x); m = extent_step(m, c.y, r.y); m = extent_step(m, c.z, r.z); m = extent_step(m, c.w, r.w);
            }
        }
        m = extent_merge(m, __shfl_xor(m, 1, 64));
        m = extent_merge(m, __shfl_xor(m, 2, 64));
        if (live && sub == 0) g.extent[5 * n + 4] = extent_merge(g.extent[5 * n + 4], m);
    }
    if (!live || !(g.mask >> sub & 1u)) return;
    float e = g.extent[5 * n + sub];
    if (sub == 2) {
        const float4 c = reinterpret_cast<const float4*>(g.cur.rotations)[n], r = reinterpret_cast<const float4*>(g.ref.rotations)[n];
        e = extent_step(e, c.x, r.x); e = extent_step(e, c.y, r.y); e = extent_step(e, c.z, r.z); e = extent_step(e, c.w, r.w);
    } else if (sub == 3) {
        e = extent_step(e, g.cur.opacity[n], g.ref.opacity[n]);
    } else {
        const float* __restrict__ c = (sub ? g.cur.scales : g.cur.xyz) + 3 * n;
        const float* __restrict__ r = (sub ? g.ref.scales : g.ref.xyz) + 3 * n;
        e = extent_step(e, c[0], r[0]); e = extent_step(e, c[1], r[1]); e = extent_step(e, c[2], r[2]);
    }
    g.extent[5 * n + sub] = e;
}


static inline const float* field_of(const fdgs_state_arrays* s, int h) {
    return h == 0 ? s->xyz : h == 1 ? s->scales : h == 2 ? s->rotations : h == 3 ? s->opacity : s->shs;
}
constexpr int STATE_WIDTH[5] = {3, 3, 4, 1, 48};

// the selected fields of up to three states: non-NULL, and on the device entry points aligned
static int check_fields(unsigned field_mask, const fdgs_state_arrays* x, const fdgs_state_arrays* y, const fdgs_state_arrays* z, bool device) {
    for (int h = 0; h < 5; h++) {
        if (!(field_mask >> h & 1u)) continue;
        const fdgs_state_arrays* s[3] = {x, y, z};
        for (int k = 0; k < 3; k++) {
            if (!s[k]) continue;
            const float* p = field_of(s[k], h);
            FDGS_REQUIRE(p, "NULL pointer (every state needs the arrays of a selected field)");
            if (device) {
                FDGS_REQUIRE(aligned_to(p, 4), "arrays must be 4-byte aligned");
                if (h == 2 || h == 4) FDGS_REQUIRE(aligned_to(p, 16), "rotations and SH must be 16-byte aligned");
            }
        }
    }
    return FDGS_OK;
}

static int check_extent(int N, unsigned field_mask, const fdgs_state_arrays* ref, const fdgs_state_arrays* cur, const float* extent, bool device) {
    FDGS_REQUIRE(N >= 0, "bad N (negative)");
    FDGS_REQUIRE(field_mask <= STATE_ALL_FIELDS, "bad field_mask (bits 0 .. 4: positions, scales, rotations, opacity, SH)");
    if (N == 0 || field_mask == 0) return FDGS_OK;
    FDGS_REQUIRE(ref && cur && extent, "NULL pointer (ref, cur and extent)");
    if (device) FDGS_REQUIRE(aligned_to(extent, 4), "extent must be 4-byte aligned");
    return check_fields(field_mask, ref, cur, nullptr, device);
}

// gather (b = NULL, w = 0) and scatter
static int check_rows(int D, const int32_t* rows, int N, unsigned field_mask, const fdgs_state_arrays* a, const fdgs_state_arrays* b, float w,
                      const fdgs_state_arrays* out, bool device) {
    FDGS_REQUIRE(D >= 0 && N >= 0, "bad D or N (negative)");
    FDGS_REQUIRE(D <= N, "bad D (more listed rows than rows)");
    FDGS_REQUIRE(field_mask <= STATE_ALL_FIELDS, "bad field_mask (bits 0 .. 4: positions, scales, rotations, opacity, SH)");
    FDGS_REQUIRE(w >= 0.f && w <= 1.f, "bad w (0 .. 1)");
    FDGS_REQUIRE(b || w == 0.f, "bad w (0 without a second state)");
    if (D == 0 || N == 0 || field_mask == 0) return FDGS_OK;
    FDGS_REQUIRE(rows, "NULL pointer (rows)");
    FDGS_REQUIRE(a && out, "NULL pointer (both sides of the copy)");
    if (device) FDGS_REQUIRE(aligned_to(rows, 4), "rows must be 4-byte aligned");
    return check_fields(field_mask, a, b, out, device);
}

// host twins only: the list is readable there
static int check_row_list(int D, const int32_t* rows, int N) {
    for (int r = 0; r < D; r++) {
        FDGS_REQUIRE(rows[r] >= 0 && rows[r] < N, "bad rows (an entry outside [0, N))");
        FDGS_REQUIRE(r == 0 || rows[r] > rows[r - 1], "bad rows (not strictly ascending)");
    }
    return FDGS_OK;
}

static int launch_rows(bool scatter, hipStream_t stream, int D, const int32_t* rows, int N, unsigned field_mask, const fdgs_state_arrays* a,
                       const fdgs_state_arrays* b, float w, const fdgs_state_arrays* out) {
    RowsArgs g{};
    g.a = *a; g.out = *out;
    if (b) g.b = *b;
    g.rows = rows; g.D = D; g.N = N; g.blend = b ? 1 : 0; g.mask = field_mask; g.w = w;
    const int blocks = cdiv(D, ROWS_TILE);
    if (scatter) { FDGS_TIMED("state_scatter", stream); hipLaunchKernelGGL(state_scatter_kernel, dim3(blocks), dim3(256), 0, stream, g); }
    else { FDGS_TIMED("state_gather", stream); hipLaunchKernelGGL(state_gather_kernel, dim3(blocks), dim3(256), 0, stream, g); }
    FDGS_LAUNCH_CHECK(scatter ? "state_scatter" : "state_gather", 0, stream);
    return FDGS_OK;
}

static int check_blend(float w, int nstreams, const fdgs_blend_stream* streams, int N, const float* rot_a, const float* rot_b, float* rot_out,
                       bool device) {
    FDGS_REQUIRE(w >= 0.f && w <= 1.f, "bad w (0 .. 1)");
    FDGS_REQUIRE(nstreams >= 0 && nstreams <= FDGS_MAX_BLEND_STREAMS, "bad nstreams (0 .. FDGS_MAX_BLEND_STREAMS)");
    FDGS_REQUIRE(N >= 0, "bad N (negative)");
    FDGS_REQUIRE(nstreams == 0 || streams, "NULL pointer (streams)");
    for (int k = 0; k < nstreams; k++) {
        if (streams[k].n_floats == 0) continue;
        FDGS_REQUIRE(streams[k].a && streams[k].b && streams[k].out, "NULL pointer (a stream needs a, b and out)");
        if (device)
            FDGS_REQUIRE(aligned_to(streams[k].a, 16) && aligned_to(streams[k].b, 16) && aligned_to(streams[k].out, 16),
                         "a stream's a, b and out must be 16-byte aligned");
    }
    const bool any_rot = rot_a || rot_b || rot_out;
    if (any_rot && N > 0) {
        FDGS_REQUIRE(rot_a && rot_b && rot_out, "NULL pointer (rotations need rot_a, rot_b and rot_out)");
        if (device) FDGS_REQUIRE(aligned_to(rot_a, 16) && aligned_to(rot_b, 16) && aligned_to(rot_out, 16), "rotations must be 16-byte aligned");
    }
    return FDGS_OK;
}

static int check_ply(int N, const float* xyz, const float* scales, const float* rotations, const float* opacity, const float* shs, const float* out) {
    FDGS_REQUIRE(N >= 0, "bad N (negative)");
    if (N == 0) return FDGS_OK;
    FDGS_REQUIRE(xyz && scales && rotations && opacity && shs && out, "NULL pointer");
    return FDGS_OK;
}

static int check_rgb8(int H, int W, int mode, const float* image, const uint8_t* out) {
    FDGS_REQUIRE(H >= 0 && W >= 0, "bad image size (negative)");
    FDGS_REQUIRE(mode == FDGS_RGB8_TRUNC || mode == FDGS_RGB8_ROUND, "bad mode (FDGS_RGB8_TRUNC | FDGS_RGB8_ROUND)");
    if (H == 0 || W == 0) return FDGS_OK;
    FDGS_REQUIRE(image && out, "NULL pointer");
    return FDGS_OK;
}
}  // namespace fdgs

using namespace fdgs;

extern "C" int fdgs_state_blend(void* stream_, float w, int nstreams, const fdgs_blend_stream* streams, int N, const float* rot_a,
                                const float* rot_b, float* rot_out) {
    const int rc = check_blend(w, nstreams, streams, N, rot_a, rot_b, rot_out, true);
    if (rc != FDGS_OK) return rc;
    BlendArgs g{};
    long long blocks = 0;
    int s = 0;
    for (int k = 0; k < nstreams; k++) {
        const unsigned long long n = streams[k].n_floats;
        if (n == 0) continue;
        g.a[s] = streams[k].a; g.b[s] = streams[k].b; g.out[s] = streams[k].out; g.n[s] = n;
        g.first_block[s++] = (int)blocks;
        blocks += (long long)(((n >> 2) + ((n & 3) ? 1 : 0) + 255) / 256);
        FDGS_REQUIRE(blocks < (1ll << 31), "streams too long for one launch");
    }
    g.rot_seg = -1;
    if (rot_a && N > 0) {
        g.a[s] = rot_a; g.b[s] = rot_b; g.out[s] = rot_out; g.n[s] = (unsigned long long)N;
        g.rot_seg = s;
        g.first_block[s++] = (int)blocks;
        blocks += cdiv(N, 256);
        FDGS_REQUIRE(blocks < (1ll << 31), "streams too long for one launch");
    }
    if (s == 0) return FDGS_OK;
    g.first_block[s] = (int)blocks;
    g.nseg = s;
    g.w = w;
    hipStream_t stream = (hipStream_t)stream_;
    { FDGS_TIMED("state_blend", stream); hipLaunchKernelGGL(state_blend_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, g); }
    FDGS_LAUNCH_CHECK("state_blend", 0, stream);
    return FDGS_OK;
}

extern "C" int fdgs_state_blend_host(float w, int nstreams, const fdgs_blend_stream* streams, int N, const float* rot_a, const float* rot_b,
                                     float* rot_out) {
    const int rc = check_blend(w, nstreams, streams, N, rot_a, rot_b, rot_out, false);
    if (rc != FDGS_OK) return rc;
    for (int k = 0; k < nstreams; k++)
        for (size_t i = 0; i < streams[k].n_floats; i++) streams[k].out[i] = blend_lerp(streams[k].a[i], streams[k].b[i], w);
    if (rot_a)
        for (size_t i = 0; i < (size_t)N; i++) blend_quat(rot_a + 4 * i, rot_b + 4 * i, w, rot_out + 4 * i);
    return FDGS_OK;
}

extern "C" int fdgs_pack_ply_rows(void* stream_, int N, const float* xyz, const float* scales, const float* rotations, const float* opacity,
                                  const float* shs, float* out) {
    const int rc = check_ply(N, xyz, scales, rotations, opacity, shs, out);
    if (rc != FDGS_OK || N == 0) return rc;
    const long long total = (long long)N * PLY_COLUMNS;
    hipStream_t stream = (hipStream_t)stream_;
    { FDGS_TIMED("pack_ply_rows", stream);
      hipLaunchKernelGGL(pack_ply_rows_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, total, xyz, scales, rotations, opacity, shs, out); }
    FDGS_LAUNCH_CHECK("pack_ply_rows", 0, stream);
    return FDGS_OK;
}

extern "C" int fdgs_pack_ply_rows_host(int N, const float* xyz, const float* scales, const float* rotations, const float* opacity,
                                       const float* shs, float* out) {
    const int rc = check_ply(N, xyz, scales, rotations, opacity, shs, out);
    if (rc != FDGS_OK || N == 0) return rc;
    const float* src[5] = {xyz, scales, rotations, opacity, shs};
    for (long long n = 0; n < N; n++)
        for (int c = 0; c < PLY_COLUMNS; c++) {
            int array;
            const long long s = ply_source(n, c, &array);
            out[n * PLY_COLUMNS + c] = array < 0 ? 0.f : src[array][s];
        }
    return FDGS_OK;
}

extern "C" int fdgs_image_rgb8(void* stream_, int H, int W, int mode, const float* image, uint8_t* out) {
    const int rc = check_rgb8(H, W, mode, image, out);
    if (rc != FDGS_OK || H == 0 || W == 0) return rc;
    const long long HW = (long long)H * W;
    const int vec_in = (HW % 4 == 0 && aligned_to(image, 16)) ? 1 : 0, vec_out = aligned_to(out, 4) ? 1 : 0;
    hipStream_t stream = (hipStream_t)stream_;
    { FDGS_TIMED("image_rgb8", stream);
      hipLaunchKernelGGL(image_rgb8_kernel, dim3(cdiv((HW + 3) / 4, 256)), dim3(256), 0, stream, HW, mode, vec_in, vec_out, image, out); }
    FDGS_LAUNCH_CHECK("image_rgb8", 0, stream);
    return FDGS_OK;
}

extern "C" int fdgs_image_rgb8_host(int H, int W, int mode, const float* image, uint8_t* out) {
    const int rc = check_rgb8(H, W, mode, image, out);
    if (rc != FDGS_OK || H == 0 || W == 0) return rc;
    const long long HW = (long long)H * W;
    for (long long p = 0; p < HW; p++)
        for (int c = 0; c < 3; c++) out[3 * p + c] = rgb8_value(image[c * HW + p], mode);
    return FDGS_OK;
}

extern "C" int fdgs_state_extent(void* stream_, int N, unsigned field_mask, const fdgs_state_arrays* ref, const fdgs_state_arrays* cur,
                                 float* extent) {
    const int rc = check_extent(N, field_mask, ref, cur, extent, true);
    if (rc != FDGS_OK || N == 0 || field_mask == 0) return rc;
    ExtentArgs g{};
    g.ref = *ref; g.cur = *cur; g.extent = extent; g.N = N; g.mask = field_mask;
    hipStream_t stream = (hipStream_t)stream_;
    { FDGS_TIMED("state_extent", stream); hipLaunchKernelGGL(state_extent_kernel, dim3(cdiv(N, ROWS_TILE)), dim3(256), 0, stream, g); }
    FDGS_LAUNCH_CHECK("state_extent", 0, stream);
    return FDGS_OK;
}

extern "C" int fdgs_state_extent_host(int N, unsigned field_mask, const fdgs_state_arrays* ref, const fdgs_state_arrays* cur, float* extent) {
    const int rc = check_extent(N, field_mask, ref, cur, extent, false);
    if (rc != FDGS_OK || N == 0 || field_mask == 0) return rc;
    for (int h = 0; h < 5; h++) {
        if (!(field_mask >> h & 1u)) continue;
        const float* r = field_of(ref, h);
        const float* c = field_of(cur, h);
        const size_t wd = STATE_WIDTH[h];
        for (size_t n = 0; n < (size_t)N; n++) {
            float e = extent[5 * n + h];
            for (size_t k = 0; k < wd; k++) e = extent_step(e, c[wd * n + k], r[wd * n + k]);
            extent[5 * n + h] = e;
        }
    }
    return FDGS_OK;
}

extern "C" int fdgs_state_gather(void* stream_, int D, const int32_t* rows, int N, unsigned field_mask, const fdgs_state_arrays* full,
                                 const fdgs_state_arrays* compact) {
    const int rc = check_rows(D, rows, N, field_mask, full, nullptr, 0.f, compact, true);
    if (rc != FDGS_OK || D == 0 || N == 0 || field_mask == 0) return rc;
    return launch_rows(false, (hipStream_t)stream_, D, rows, N, field_mask, full, nullptr, 0.f, compact);
}

extern "C" int fdgs_state_gather_host(int D, const int32_t* rows, int N, unsigned field_mask, const fdgs_state_arrays* full,
                                      const fdgs_state_arrays* compact) {
    int rc = check_rows(D, rows, N, field_mask, full, nullptr, 0.f, compact, false);
    if (rc != FDGS_OK || D == 0 || N == 0 || field_mask == 0) return rc;
    if ((rc = check_row_list(D, rows, N)) != FDGS_OK) return rc;
    for (int h = 0; h < 5; h++) {
        if (!(field_mask >> h & 1u)) continue;
        const float* src = field_of(full, h);
        float* dst = const_cast<float*>(field_of(compact, h));
        const size_t wd = STATE_WIDTH[h];
        for (size_t r = 0; r < (size_t)D; r++) memcpy(dst + wd * r, src + wd * (size_t)rows[r], 4 * wd);
    }
    return FDGS_OK;
}

extern "C" int fdgs_state_scatter(void* stream_, int D, const int32_t* rows, int N, unsigned field_mask, const fdgs_state_arrays* a,
                                  const fdgs_state_arrays* b, float w, const fdgs_state_arrays* out) {
    const int rc = check_rows(D, rows, N, field_mask, a, b, w, out, true);
    if (rc != FDGS_OK || D == 0 || N == 0 || field_mask == 0) return rc;
    return launch_rows(true, (hipStream_t)stream_, D, rows, N, field_mask, a, b, w, out);
}

extern "C" int fdgs_state_scatter_host(int D, const int32_t* rows, int N, unsigned field_mask, const fdgs_state_arrays* a,
                                       const fdgs_state_arrays* b, float w, const fdgs_state_arrays* out) {
    int rc = check_rows(D, rows, N, field_mask, a, b, w, out, false);
    if (rc != FDGS_OK || D == 0 || N == 0 || field_mask == 0) return rc;
    if ((rc = check_row_list(D, rows, N)) != FDGS_OK) return rc;
    for (int h = 0; h < 5; h++) {
        if (!(field_mask >> h & 1u)) continue;
        const float* pa = field_of(a, h);
        const float* pb = b ? field_of(b, h) : nullptr;
        float* dst = const_cast<float*>(field_of(out, h));
        const size_t wd = STATE_WIDTH[h];
        for (size_t r = 0; r < (size_t)D; r++) {
            float* o = dst + wd * (size_t)rows[r];
            if (!pb) memcpy(o, pa + wd * r, 4 * wd);
            else if (h == 2) blend_quat(pa + 4 * r, pb + 4 * r, w, o);
            else for (size_t k = 0; k < wd; k++) o[k] = blend_lerp(pa[wd * r + k], pb[wd * r + k], w);
        }
    }
    return FDGS_OK;
}
