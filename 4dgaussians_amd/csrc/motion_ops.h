// motion_ops.h -- the arithmetic of the motion-vector pass, ONE function per operation for the device kernel and the host entry point (the
// idiom of playback_ops.h): fdgs_motion_rows / fdgs_motion_resolve and their *_host twins call exactly these.
//
// Every function is compiled with floating-point contraction OFF and uses only * + - / and compares: every float32 operation below is ONE
// IEEE operation in the order written, so the device result equals the host result bit for bit (tests/test_gpu_motion.py) and a numpy
// restatement in np.float32 equals both (tests/test_motion_host.py).  Matrices are in the layout the rasterizer reads (view_xform in
// gs_math.h): element m[4 * j + i].
//
//   motion_pix        pixel coordinate k (0: x, 1: y) of point p in an image S pixels wide (k = 0) / high (k = 1), the rasterizer's own
//                     convention (FDGS_W_EPS, ndc2pix):
//                       h = m[k] * p0;  h = h + m[4 + k] * p1;  h = h + m[8 + k] * p2;  h = h + m[12 + k]
//                       w = m[3] * p0;  w = w + m[7] * p1;      w = w + m[11] * p2;     w = w + m[15]
//                       d = w + 1e-7f;  r = 1.0f / d;  x = h * r
//                       t = x + 1.0f;  t = t * (float)S;  t = t - 1.0f;  pix = t * 0.5f
//   motion_zview      v[2] * p0 + v[6] * p1 + v[10] * p2 + v[14], summed left to right: the depth the near cull looks at
//   motion_row        ok = zview(at) > 0.2f && zview(toward) > 0.2f (the rasterizer's near cull, in BOTH views);
//                     out = ok ? (pix_x(toward) - pix_x(at), pix_y(toward) - pix_y(at), 1) : (0, 0, 1).  Add out to a pixel's coordinates in
//                     THIS frame to find the same surface point in the TOWARD frame.  The third value is always 1: blended, it is the coverage.
//   motion_resolve_px ok = a > min_alpha;  mx = ok ? rx / a : 0, my the same (a NaN a fails the compare: zeros)
#pragma once
#include "playback_ops.h"

namespace fdgs {

constexpr float MOTION_NEAR = 0.2f;          // FDGS_NEAR_CULL of gs_math.h
constexpr float MOTION_W_EPS = 0.0000001f;   // FDGS_W_EPS

FDGS_HD inline float motion_pix(const float* m, const float* p, int S, int k) {
#pragma clang fp contract(off)
    float h = m[k] * p[0];
    const float h1 = m[4 + k] * p[1];
    h = h + h1;
    const float h2 = m[8 + k] * p[2];
    h = h + h2;
    h = h + m[12 + k];
    float w = m[3] * p[0];
    const float w1 = m[7] * p[1];
    w = w + w1;
    const float w2 = m[11] * p[2];
    w = w + w2;
    w = w + m[15];
    const float d = w + MOTION_W_EPS;
    const float r = 1.0f / d;
    const float x = h * r;
    float t = x + 1.0f;
    t = t * (float)S;
    t = t - 1.0f;
    return t * 0.5f;
}

FDGS_HD inline float motion_zview(const float* v, const float* p) {
#pragma clang fp contract(off)
    float z = v[2] * p[0];
    const float z1 = v[6] * p[1];
    z = z + z1;
    const float z2 = v[10] * p[2];
    z = z + z2;
    return z + v[14];
}

FDGS_HD inline void motion_row(const float* view_at, const float* proj_at, const float* p_at, const float* view_to, const float* proj_to,
                               const float* p_to, int W, int H, float* out3) {
#pragma clang fp contract(off)
    const bool ok = motion_zview(view_at, p_at) > MOTION_NEAR && motion_zview(view_to, p_to) > MOTION_NEAR;
    const float dx = motion_pix(proj_to, p_to, W, 0) - motion_pix(proj_at, p_at, W, 0);
    const float dy = motion_pix(proj_to, p_to, H, 1) - motion_pix(proj_at, p_at, H, 1);
    out3[0] = ok ? dx : 0.f;
    out3[1] = ok ? dy : 0.f;
    out3[2] = 1.0f;
}

FDGS_HD inline void motion_resolve_px(float rx, float ry, float a, float min_alpha, float* mx, float* my) {
#pragma clang fp contract(off)
    const bool ok = a > min_alpha;
    const float qx = rx / a;
    const float qy = ry / a;
    *mx = ok ? qx : 0.f;
    *my = ok ? qy : 0.f;
}

}  // namespace fdgs
