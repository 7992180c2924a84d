// playback_ops.h -- the arithmetic of the playback operations, ONE function per operation for the device kernel and the host entry point
// (the idiom of spatial_keys.h): fdgs_state_blend / fdgs_pack_ply_rows / fdgs_image_rgb8 and their *_host twins call exactly these.
//
// Every function is compiled with floating-point contraction OFF (no fused multiply-add is formed from a * b + c), uses plain `/` and sqrtf
// (both correctly rounded in the library's build) and no other library function: every float32 operation below is ONE IEEE operation in the
// order written, so the device result equals the host result bit for bit.  That equality is what tests/test_gpu_playback.py asserts.
//
//   blend_lerp   out = a + w * (b - a)                                                     three roundings
//   blend_quat   s = dot(a, b) < 0 ? -1 : 1;  q = a + w * (s * b - a);  out = q / max(sqrt(q . q), 1e-12)
//                dot product and squared norm summed in index order 0, 1, 2, 3 (s * b is exact)
//   extent_step  e = max(e, |cur - ref|), +inf when the difference is a NaN               (fdgs_state_extent; fdgs_state_scatter blends
//                                                                                          with blend_lerp / blend_quat, fdgs_state_gather copies)
//   ply_source   which input float lands in column c of a row of io.write_ply_vertices' table (pure data movement)
//   rgb8_value   mode 0: (uint8)(255.f * min(max(x, 0), 1))           the reference's to8b: one rounding, truncation
//                mode 1: t = x * 255.f; t = t + 0.5f; clamp to [0, 255]; truncate        torchvision.utils.save_image: two roundings
//                NaN inputs are unspecified in both modes.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/fdgs.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FDGS_HD __host__ __device__
#else
#define FDGS_HD
#endif

namespace fdgs {

FDGS_HD inline float blend_lerp(float a, float b, float w) {
#pragma clang fp contract(off)
    const float d = b - a;
    const float m = w * d;
    return a + m;
}

// a, b: unit quaternions (4 floats each); out may alias neither
FDGS_HD inline void blend_quat(const float* a, const float* b, float w, float* out) {
#pragma clang fp contract(off)
    float dot = a[0] * b[0];
    dot = dot + a[1] * b[1];
    dot = dot + a[2] * b[2];
    dot = dot + a[3] * b[3];
    const float s = dot < 0.f ? -1.f : 1.f;
    float q[4];
    for (int k = 0; k < 4; k++) {
        const float sb = s * b[k];
        const float d = sb - a[k];
        const float m = w * d;
        q[k] = a[k] + m;
    }
    float nn = q[0] * q[0];
    nn = nn + q[1] * q[1];
    nn = nn + q[2] * q[2];
    nn = nn + q[3] * q[3];
    float len = sqrtf(nn);
    len = len > 1e-12f ? len : 1e-12f;
    for (int k = 0; k < 4; k++) out[k] = q[k] / len;
}

// one component of fdgs_state_extent: the running maximum e after |cur - ref|; a NaN difference makes it +inf.  The result of a whole row
// does not depend on the order of its components (a maximum; +inf absorbs), so lanes may each fold a part from +0 and the parts be
// folded into e by extent_merge: the bits are those of the sequential loop (for every e that is not itself a NaN; the caller zero-fills
// the array and nothing here ever writes one).
FDGS_HD inline float extent_step(float e, float cur, float ref) {
#pragma clang fp contract(off)
    const float d = cur - ref;
    const float m = fabsf(d);
    if (m != m) return INFINITY;
    return m > e ? m : e;
}

// e after a partial maximum m (never NaN: it came from extent_step started at +0)
FDGS_HD inline float extent_merge(float e, float m) { return m > e ? m : e; }

constexpr int PLY_COLUMNS = 62;     // x y z | nx ny nz | f_dc_0..2 | f_rest_0..44 | opacity | scale_0..2 | rot_0..3

// column c (0 .. 61) of row n of the vertex table: *array = 0 xyz, 1 scales, 2 rotations, 3 opacity, 4 shs, -1 the constant zero (normals);
// returns the float index inside that array.  f_rest_{ch * 15 + k} = shs[n, 1 + k, ch]: the reference's transpose(1, 2).flatten(start_dim=1).
FDGS_HD inline long long ply_source(long long n, int c, int* array) {
    if (c < 3) { *array = 0; return 3 * n + c; }
    if (c < 6) { *array = -1; return 0; }
    if (c < 9) { *array = 4; return 48 * n + (c - 6); }
    if (c < 54) {
        const int r = c - 9, ch = r / 15, k = r - 15 * ch;
        *array = 4;
        return 48 * n + 3 * (1 + k) + ch;
    }
    if (c < 55) { *array = 3; return n; }
    if (c < 58) { *array = 1; return 3 * n + (c - 55); }
    *array = 2;
    return 4 * n + (c - 58);
}

FDGS_HD inline uint8_t rgb8_value(float x, int mode) {
#pragma clang fp contract(off)
    if (mode == 0) {
        float c = x > 0.f ? x : 0.f;
        c = c < 1.f ? c : 1.f;
        const float t = 255.f * c;
        return (uint8_t)(int)t;
    }
    float t = x * 255.f;
    t = t + 0.5f;
    t = t > 0.f ? t : 0.f;
    t = t < 255.f ? t : 255.f;
    return (uint8_t)(int)t;
}

}  // namespace fdgs
