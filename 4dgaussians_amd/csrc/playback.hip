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

static inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

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
