// spatial_keys.h -- the space-filling-curve key of one position, ONE function for the device kernel and the host entry point.
//
// Restates fdgs.densify._quantise + hilbert_keys / morton_keys (the torch expressions, which stay the oracle) operation for operation:
//   lo = min(a, b), hi = max(a, b) over the two bound rows;  d = max(hi - lo, 1e-20f);  num = p - lo          (one f32 operation each)
//   q  = (float)((double)num / (double)d)    the correctly rounded f32 quotient: a double quotient of two f32 values rounded once more to
//                                            f32 equals the IEEE f32 division (53 >= 2 * 24 + 2), whatever the compiler makes of f32 `/`
//   c  = trunc(clamp(q * 2^bits, 0, 2^bits - 1))                                                              (the product is exact)
//   Hilbert: Skilling's transpose loop, the Gray step, then spread(X0) << 2 | spread(X1) << 1 | spread(X2)
//   Morton : spread(x) | spread(y) << 1 | spread(z) << 2
// bits = 1 .. 10, keys use 3 * bits bits.  A non-finite coordinate goes to cell 0 of its axis (the torch expressions are undefined there).
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

FDGS_HD inline uint32_t curve_spread3(uint32_t v) {      // 10 bits abc... -> a00b00c00...
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

FDGS_HD inline uint32_t curve_cell(float p, float a, float b, int bits) {
    const float lo = a < b ? a : b, hi = a < b ? b : a;
    float d = hi - lo;
    d = d > 1e-20f ? d : 1e-20f;
    const float num = p - lo;
    const float q = (float)((double)num / (double)d);
    const float v = q * (float)(1u << bits), top = (float)((1u << bits) - 1u);
    if (!(fabsf(p) <= 3.402823466e38f)) return 0u;      // inf / NaN
    const float c = v > 0.f ? (v < top ? v : top) : 0.f;  // (NaN -> 0)
    return (uint32_t)c;
}

// bounds = two opposite corners of the box, rows in either order
FDGS_HD inline uint32_t curve_key(float x, float y, float z, const float* bounds, int curve, int bits) {
    uint32_t X0 = curve_cell(x, bounds[0], bounds[3], bits);
    uint32_t X1 = curve_cell(y, bounds[1], bounds[4], bits);
    uint32_t X2 = curve_cell(z, bounds[2], bounds[5], bits);
    if (curve == FDGS_CURVE_MORTON) return curve_spread3(X0) | (curve_spread3(X1) << 1) | (curve_spread3(X2) << 2);
    for (uint32_t Q = 1u << (bits - 1); Q > 1u; Q >>= 1) {      // inverse undo of the excess work
        const uint32_t P = Q - 1u;
        X0 = (X0 & Q) ? X0 ^ P : X0;
        {
            const uint32_t t = (X0 ^ X1) & P;
            if (X1 & Q) X0 ^= P; else { X0 ^= t; X1 ^= t; }
        }
        {
            const uint32_t t = (X0 ^ X2) & P;
            if (X2 & Q) X0 ^= P; else { X0 ^= t; X2 ^= t; }
        }
    }
    X1 ^= X0;                                                   // Gray encode
    X2 ^= X1;
    uint32_t t = 0u;
    for (uint32_t Q = 1u << (bits - 1); Q > 1u; Q >>= 1)
        if (X2 & Q) t ^= Q - 1u;
    X0 ^= t; X1 ^= t; X2 ^= t;
    return (curve_spread3(X0) << 2) | (curve_spread3(X1) << 1) | curve_spread3(X2);
}

}  // namespace fdgs
