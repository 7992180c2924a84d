// compose_ops.h -- the arithmetic of placing a baked state in a common world, ONE function per operation for the device kernel and the
// host entry point (the idiom of playback_ops.h): fdgs_state_place and fdgs_state_place_host call exactly these.
//
// A placement (fdgs_placement) is a similarity transform: scale s > 0, rotation R (row-major 3x3) with its unit quaternion qR in the
// rasterizer's (r, x, y, z) order, shift d, and the matrices M1 [3x3], M2 [5x5], M3 [7x7] (row-major [j][k]) that mix the coefficients
// of one SH band under R.  Every function is compiled with floating-point contraction OFF and uses plain `*`, `+` and `-` only: every
// float32 operation below is ONE IEEE operation in the order written, so the device result equals the host result bit for bit.
//
//   place_point   t_k = s * p_k;  y_i = R[i][0] * t_0 + R[i][1] * t_1 + R[i][2] * t_2 (summed left to right);  out_i = y_i + d_i
//                 scale, rotate, shift: the order of the reference's merge script
//   place_scale   out_k = s * scale_k                                  (activated state: scales are lengths)
//   place_quat    out = qR (x) q, the Hamilton product; each component four products summed in the written order, no renormalisation
//                   r = r1 r2 - x1 x2 - y1 y2 - z1 z2        x = r1 x2 + x1 r2 + y1 z2 - z1 y2
//                   y = r1 y2 - x1 z2 + y1 r2 + z1 x2        z = r1 z2 + x1 y2 - y1 x2 + z1 r2             (1 = qR, 2 = q)
//   place_sh      one colour channel (16 coefficients `stride` floats apart): band 0 is copied; band l = 1 .. 3 occupies coefficients
//                 l * l .. l * l + 2 l:  out[k] = sum_j in[j] * M_l[j][k], acc = +0, then acc = acc + in[j] * M_l[j][k] for j ascending.
//                 FDGS_PLACE_POINTS copies the bands instead (the reference script's semantics).  In both modes the bands above
//                 sh_degree are written as +0.0.
//   place_row_*   what one row of a field becomes: the value of state a, or blend_lerp / blend_quat (playback_ops.h) of a and b at w
//                 when b is given, then placed.  Opacity is never changed by a placement.
#pragma once
#include "playback_ops.h"

namespace fdgs {

FDGS_HD inline void place_point(const fdgs_placement& p, const float* in, float* out) {
#pragma clang fp contract(off)
    const float t0 = p.scale * in[0], t1 = p.scale * in[1], t2 = p.scale * in[2];
    for (int i = 0; i < 3; i++) {
        float y = p.rot[3 * i] * t0;
        y = y + p.rot[3 * i + 1] * t1;
        y = y + p.rot[3 * i + 2] * t2;
        out[i] = y + p.shift[i];
    }
}

FDGS_HD inline void place_scale(const fdgs_placement& p, const float* in, float* out) {
#pragma clang fp contract(off)
    for (int k = 0; k < 3; k++) out[k] = p.scale * in[k];
}

// a = qR, b = the row's quaternion; out may alias neither
FDGS_HD inline void place_quat(const float* a, const float* b, float* out) {
#pragma clang fp contract(off)
    float r = a[0] * b[0];
    r = r - a[1] * b[1];
    r = r - a[2] * b[2];
    r = r - a[3] * b[3];
    float x = a[0] * b[1];
    x = x + a[1] * b[0];
    x = x + a[2] * b[3];
    x = x - a[3] * b[2];
    float y = a[0] * b[2];
    y = y - a[1] * b[3];
    y = y + a[2] * b[0];
    y = y + a[3] * b[1];
    float z = a[0] * b[3];
    z = z + a[1] * b[2];
    z = z - a[2] * b[1];
    z = z + a[3] * b[0];
    out[0] = r; out[1] = x; out[2] = y; out[3] = z;
}

template <int L>
FDGS_HD inline void place_sh_band(const float* M, bool mix, bool live, const float* in, float* out, int stride) {
#pragma clang fp contract(off)
    constexpr int W = 2 * L + 1, first = L * L;
#pragma unroll
    for (int k = 0; k < W; k++) {
        float acc = 0.f;
        if (live && mix) {
#pragma unroll
            for (int j = 0; j < W; j++) acc = acc + in[(first + j) * stride] * M[j * W + k];
        } else if (live) {
            acc = in[(first + k) * stride];
        }
        out[(first + k) * stride] = acc;
    }
}

// in, out: the 16 coefficients of ONE colour channel, `stride` floats apart; out may not alias in
FDGS_HD inline void place_sh(const fdgs_placement& p, const float* in, float* out, int stride) {
    const bool mix = p.mode == FDGS_PLACE_RIGID;
    out[0] = in[0];
    place_sh_band<1>(p.sh1, mix, p.sh_degree >= 1, in, out, stride);
    place_sh_band<2>(p.sh2, mix, p.sh_degree >= 2, in, out, stride);
    place_sh_band<3>(p.sh3, mix, p.sh_degree >= 3, in, out, stride);
}

// ---- one row of a field: blended when b != nullptr, then placed ----
FDGS_HD inline void place_row_xyz(const fdgs_placement& p, const float* a, const float* b, float w, float* out) {
    float v[3];
    for (int k = 0; k < 3; k++) v[k] = b ? blend_lerp(a[k], b[k], w) : a[k];
    place_point(p, v, out);
}

FDGS_HD inline void place_row_scales(const fdgs_placement& p, const float* a, const float* b, float w, float* out) {
    float v[3];
    for (int k = 0; k < 3; k++) v[k] = b ? blend_lerp(a[k], b[k], w) : a[k];
    place_scale(p, v, out);
}

// v: the row's (blended) quaternion
FDGS_HD inline void place_rotation(const fdgs_placement& p, const float* v, float* out) {
    if (p.mode == FDGS_PLACE_RIGID) place_quat(p.quat, v, out);
    else for (int k = 0; k < 4; k++) out[k] = v[k];
}

FDGS_HD inline void place_row_rotation(const fdgs_placement& p, const float* a, const float* b, float w, float* out) {
    float v[4];
    if (b) blend_quat(a, b, w, v);
    else for (int k = 0; k < 4; k++) v[k] = a[k];
    place_rotation(p, v, out);
}

FDGS_HD inline float place_row_opacity(const float* a, const float* b, float w) { return b ? blend_lerp(a[0], b[0], w) : a[0]; }

}  // namespace fdgs
