// motion.hip -- motion vectors and coverage of a finished forward-only frame, beside the rasterizer: the two small kernels around ONE extra
// blend pass (fdgs_render_fwd on the frame's own geom / binning / img, see include/fdgs.h at fdgs_geom_field).
//
// Two memory-bound streaming kernels (no LDS, no atomics); the arithmetic of each is ONE host/device function of motion_ops.h that the
// *_host entry points below call as well, compiled without contraction: the device result is the host result bit for bit.
//
//   fdgs_motion_rows     one row per lane: 24 bytes in (the row's position in this frame and in the toward frame), 12 or 16 bytes out (the
//                        row's screen-space motion and a 1: the colour record the blend reads).  The four matrices are the same for every
//                        lane: they are read through uniform addresses, once per workgroup.  One float4 store per lane when the output has
//                        four floats per row and is 16-byte aligned (recC is), scalar stores otherwise.
//   fdgs_motion_resolve  one thread per four pixels: motion = raw.xy / raw.z where raw.z > min_alpha, alpha = raw.z.  A plane that starts on
//                        16 bytes moves as float4s; the others, and the last H * W % 4 pixels, as scalars.
#include "common.h"
#include "motion_ops.h"

namespace fdgs {

__global__ void __launch_bounds__(256) motion_rows_kernel(int N, const float* __restrict__ xyz_at, const float* __restrict__ xyz_to,
                                                          const float* __restrict__ view_at, const float* __restrict__ proj_at,
                                                          const float* __restrict__ view_to, const float* __restrict__ proj_to, int W, int H,
                                                          float* __restrict__ out, int out_stride, int vec_out) {
    float va[16], pa[16], vt[16], pt[16];       // (uniform addresses: scalar loads, once per wave)
#pragma unroll
    for (int k = 0; k < 16; k++) { va[k] = view_at[k]; pa[k] = proj_at[k]; vt[k] = view_to[k]; pt[k] = proj_to[k]; }
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= N) return;
    const float a[3] = {xyz_at[3 * row], xyz_at[3 * row + 1], xyz_at[3 * row + 2]};
    const float b[3] = {xyz_to[3 * row], xyz_to[3 * row + 1], xyz_to[3 * row + 2]};
    float m[3];
    motion_row(va, pa, a, vt, pt, b, W, H, m);
    if (vec_out) {
        reinterpret_cast<float4*>(out)[row] = make_float4(m[0], m[1], m[2], 0.f);
        return;
    }
    float* o = out + (long long)out_stride * row;
    o[0] = m[0]; o[1] = m[1]; o[2] = m[2];
    if (out_stride == 4) o[3] = 0.f;
}

// bit c of `vec`: plane c (raw 0, 1, 2, motion 0, 1, alpha) starts on 16 bytes
__global__ void __launch_bounds__(256) motion_resolve_kernel(long long HW, float min_alpha, unsigned vec, const float* __restrict__ raw,
                                                             float* __restrict__ motion, float* __restrict__ alpha) {
    const long long p0 = 4 * ((long long)blockIdx.x * 256 + threadIdx.x);
    if (p0 >= HW) return;
    const int cnt = HW - p0 < 4 ? (int)(HW - p0) : 4;
    float v[3][4] = {};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float* src = raw + c * HW + p0;
        if ((vec >> c & 1u) && cnt == 4) {
            const float4 t = *reinterpret_cast<const float4*>(src);
            v[c][0] = t.x; v[c][1] = t.y; v[c][2] = t.z; v[c][3] = t.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < cnt) v[c][k] = src[k];
        }
    }
    float o[3][4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        motion_resolve_px(v[0][k], v[1][k], v[2][k], min_alpha, &o[0][k], &o[1][k]);
        o[2][k] = v[2][k];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float* dst = (c < 2 ? motion + c * HW : alpha) + p0;
        if ((vec >> (3 + c) & 1u) && cnt == 4) {
            *reinterpret_cast<float4*>(dst) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < cnt) dst[k] = o[c][k];
        }
    }
}

static int check_motion_rows(int N, const float* xyz_at, const float* xyz_to, const float* view_at, const float* proj_at, const float* view_to,
                             const float* proj_to, int W, int H, const float* out, int out_stride, bool device) {
    FDGS_REQUIRE(N >= 0, "bad N (negative)");
    FDGS_REQUIRE(out_stride == 3 || out_stride == 4, "bad out_stride (3 or 4 floats per row)");
    FDGS_REQUIRE(W >= 1 && H >= 1, "bad image size (W and H at least 1)");
    if (N == 0) return FDGS_OK;
    FDGS_REQUIRE(xyz_at && xyz_to && out, "NULL pointer (xyz_at, xyz_toward and out)");
    FDGS_REQUIRE(view_at && proj_at && view_to && proj_to, "NULL pointer (the four matrices)");
    if (device)
        FDGS_REQUIRE(aligned_to(xyz_at, 4) && aligned_to(xyz_to, 4) && aligned_to(out, 4) && aligned_to(view_at, 4) && aligned_to(proj_at, 4) &&
                         aligned_to(view_to, 4) && aligned_to(proj_to, 4), "arrays must be 4-byte aligned");
    return FDGS_OK;
}

static int check_motion_resolve(int H, int W, const float* raw, const float* motion, const float* alpha, bool device) {
    FDGS_REQUIRE(W >= 1 && H >= 1, "bad image size (W and H at least 1)");
    FDGS_REQUIRE(raw && motion && alpha, "NULL pointer (raw, motion and alpha)");
    if (device) FDGS_REQUIRE(aligned_to(raw, 4) && aligned_to(motion, 4) && aligned_to(alpha, 4), "images must be 4-byte aligned");
    return FDGS_OK;
}
}  // namespace fdgs

using namespace fdgs;

extern "C" int fdgs_motion_rows(void* stream_, int N, const float* xyz_at, const float* xyz_toward, const float* view_at, const float* proj_at,
                                const float* view_toward, const float* proj_toward, int W, int H, float* out, int out_stride) {
    const int rc = check_motion_rows(N, xyz_at, xyz_toward, view_at, proj_at, view_toward, proj_toward, W, H, out, out_stride, true);
    if (rc != FDGS_OK || N == 0) return rc;
    const int vec_out = (out_stride == 4 && aligned_to(out, 16)) ? 1 : 0;
    hipStream_t stream = (hipStream_t)stream_;
    { FDGS_TIMED("motion_rows", stream);
      hipLaunchKernelGGL(motion_rows_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, N, xyz_at, xyz_toward, view_at, proj_at, view_toward,
                         proj_toward, W, H, out, out_stride, vec_out); }
    FDGS_LAUNCH_CHECK("motion_rows", 0, stream);
    return FDGS_OK;
}

extern "C" int fdgs_motion_rows_host(int N, const float* xyz_at, const float* xyz_toward, const float* view_at, const float* proj_at,
                                     const float* view_toward, const float* proj_toward, int W, int H, float* out, int out_stride) {
    const int rc = check_motion_rows(N, xyz_at, xyz_toward, view_at, proj_at, view_toward, proj_toward, W, H, out, out_stride, false);
    if (rc != FDGS_OK) return rc;
    for (size_t n = 0; n < (size_t)N; n++) {
        float* o = out + (size_t)out_stride * n;
        motion_row(view_at, proj_at, xyz_at + 3 * n, view_toward, proj_toward, xyz_toward + 3 * n, W, H, o);
        if (out_stride == 4) o[3] = 0.f;
    }
    return FDGS_OK;
}

extern "C" int fdgs_motion_resolve(void* stream_, int H, int W, float min_alpha, const float* raw, float* motion, float* alpha) {
    const int rc = check_motion_resolve(H, W, raw, motion, alpha, true);
    if (rc != FDGS_OK) return rc;
    const long long HW = (long long)H * W;
    const float* planes[6] = {raw, raw + HW, raw + 2 * HW, motion, motion + HW, alpha};
    unsigned vec = 0;
    for (int c = 0; c < 6; c++) vec |= aligned_to(planes[c], 16) ? 1u << c : 0u;
    hipStream_t stream = (hipStream_t)stream_;
    { FDGS_TIMED("motion_resolve", stream);
      hipLaunchKernelGGL(motion_resolve_kernel, dim3(cdiv((HW + 3) / 4, 256)), dim3(256), 0, stream, HW, min_alpha, vec, raw, motion, alpha); }
    FDGS_LAUNCH_CHECK("motion_resolve", 0, stream);
    return FDGS_OK;
}

extern "C" int fdgs_motion_resolve_host(int H, int W, float min_alpha, const float* raw, float* motion, float* alpha) {
    const int rc = check_motion_resolve(H, W, raw, motion, alpha, false);
    if (rc != FDGS_OK) return rc;
    const long long HW = (long long)H * W;
    for (long long p = 0; p < HW; p++) {
        motion_resolve_px(raw[p], raw[HW + p], raw[2 * HW + p], min_alpha, &motion[p], &motion[HW + p]);
        alpha[p] = raw[2 * HW + p];
    }
    return FDGS_OK;
}
