// hexplane_ops.h -- the index arithmetic of the HexPlane lookup, ONE function per operation for every deformation kernel, the probe
// fdgs_hexplane_cells and its host twin fdgs_hexplane_cells_host (the idiom of playback_ops.h / spatial_keys.h).
//
// The texel cell of a Gaussian is integer work: the bar is equality with the reference's float32 elementwise arithmetic (scene/hexplane.py:19-20
// normalize_aabb, then F.grid_sample's un-normalisation with align_corners=True, padding_mode='border').  Every function is compiled with
// floating-point contraction OFF (no fused multiply-add is formed from a * b + c) and uses, beside `+ - *`, only fminf / fmaxf / floorf, which
// are exact: every float32 operation below is ONE IEEE operation in the order written, so the device result equals the host result, and both
// equal torch's, bit for bit.  tests/test_hexplane_cells_host.py pins the host twin to F.grid_sample through tests/golden/hexplane_cells.npz,
// tests/test_gpu_hexplane_cells.py asserts device == host.
//
//   query_coord   d = x - aabb0;  m = d * inv2;  q = m - 1                                 three roundings
//                 (inv2 = 2 / (aabb1 - aabb0) is the reference's own float32 division, done once on the host: aabb_scale in deform_layers.h.
//                  Contracted to fma(d, inv2, -1) -- one rounding fewer -- the cell differs on ~2 % of coordinates within 8 ulps of a boundary.)
//   axis_sample   hi = size - 1;  s = coord + 1;  h = s * 0.5 (exact);  p = h * hi
//                 dscale = 0 < p < hi ? 0.5 * hi : 0          d pixel / d coord, 0 where the border clamp is active
//                 p = min(max(p, 0), hi);  f = floor(p);  i0 = (int)f;  i1 = min(i0 + 1, size - 1);  w1 = p - f (exact);  w0 = 1 - w1
//                 NaN coordinates are unspecified.
//   hexplane_cells_row   what the probe and its twin write for one Gaussian: the four query coordinates (time is never normalised) and, per
//                 level and axis, (i0, i1), w1 and dscale.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/fdgs.h"

#ifndef FDGS_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define FDGS_HD __host__ __device__
#else
#define FDGS_HD
#endif
#endif
#define FDGS_HD_INLINE FDGS_HD inline __attribute__((always_inline))

namespace fdgs {

struct AxisSample {
    int i0, i1;
    float w0, w1, dscale;  // dscale = d pixel / d coord, 0 where the border clamp is active
};

// normalize_aabb (scene/hexplane.py:19-20): aabb0 = the "max" row of the reference's aabb (the axis is flipped), inv2 = 2 / (aabb1 - aabb0)
FDGS_HD_INLINE float query_coord(float x, float aabb0, float inv2) {
#pragma clang fp contract(off)
    const float d = x - aabb0;
    const float m = d * inv2;
    return m - 1.0f;
}

// grid_sample(align_corners=True, padding_mode='border') un-normalisation (scene/hexplane.py:39-43)
FDGS_HD_INLINE AxisSample axis_sample(float coord, int size) {
#pragma clang fp contract(off)
    AxisSample s;
    const float hi = (float)(size - 1);
    float p = ((coord + 1.f) * 0.5f) * hi;
    s.dscale = (p > 0.f && p < hi) ? 0.5f * hi : 0.f;
    p = fminf(fmaxf(p, 0.f), hi);
    const float f = floorf(p);
    s.i0 = (int)f;
    s.i1 = s.i0 + 1 < size ? s.i0 + 1 : size - 1;
    s.w1 = p - f;
    s.w0 = 1.f - s.w1;
    return s;
}

// row n of fdgs_hexplane_cells: cells [L][4][2], w1 [L][4], dscale [L][4], q [4] of this Gaussian (inv2: aabb_scale of p.aabb)
FDGS_HD inline void hexplane_cells_row(const fdgs_deform_params& p, const float* inv2, size_t n, int32_t* cells, float* w1, float* dscale, float* q) {
#pragma clang fp contract(off)
    for (int i = 0; i < 3; i++) q[i] = query_coord(p.xyz[3 * n + i], p.aabb[i], inv2[i]);
    q[3] = p.time ? p.time[n] : p.time_scalar;
    for (int lvl = 0; lvl < p.L; lvl++)
        for (int ax = 0; ax < 4; ax++) {
            const AxisSample s = axis_sample(q[ax], p.res[lvl][ax]);
            cells[(lvl * 4 + ax) * 2] = s.i0;
            cells[(lvl * 4 + ax) * 2 + 1] = s.i1;
            w1[lvl * 4 + ax] = s.w1;
            dscale[lvl * 4 + ax] = s.dscale;
        }
}

}  // namespace fdgs
