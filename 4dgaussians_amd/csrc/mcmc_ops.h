// mcmc_ops.h -- the arithmetic of MCMC densification (3DGS-MCMC, Kheradmand et al. 2024), ONE function per operation, written for device kernels
// and for the host entry points fdgs_mcmc_*_host of mcmc.hip (the idiom of playback_ops.h / spatial_keys.h).  The definitions are stated in
// include/fdgs.h ("MCMC densification"); this file is their only implementation.
//
//   philox4x32_10     the generator of Salmon et al. (SC'11), ten rounds: integer arithmetic only, the same words everywhere
//   mcmc_weight       the integer sampling weight of a row (0 = dead), from the float32 opacity expression of the prune plan (densify.hip)
//   mcmc_draw         draw k: a 64-bit Philox word -> mulhi64 with the total -> the first row whose inclusive sum exceeds it
//   mcmc_relocation   x_o', x_s' of a source drawn `count` times: the whole chain in DOUBLE, rounded to float32 once
//   mcmc_normals3     three standard normals of (row, iteration): Box-Muller on Philox words
//   mcmc_noise_row    xyz + (R diag(s^2) R^T) xi * g * lr: in DOUBLE as well, rounded by the final add
//
// The float32 functions are compiled with floating-point contraction OFF: every operation is ONE IEEE operation in the order written, so a
// function gives the same bits wherever it is inlined.  expf / logf / cosf / sinf (float32) and exp / log / log1p / expm1 (double) are the platform's: host and device agree to their
// last units, not bit for bit -- except where a double result is rounded to float32 once (mcmc_relocation), where a disagreement needs the
// double value within ~1e-16 relative of a float32 rounding boundary.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/fdgs.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FDGS_MCMC_HD __host__ __device__
#else
#define FDGS_MCMC_HD
#endif

namespace fdgs {

// ---- Philox4x32-10 ------------------------------------------------------------------------------------------------------------------------
FDGS_MCMC_HD inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* out) {
    for (int round = 0; round < 10; round++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

FDGS_MCMC_HD inline uint64_t mcmc_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// ---- sampling -----------------------------------------------------------------------------------------------------------------------------
// sigmoid as the prune plan evaluates it (densify.hip: classify)
FDGS_MCMC_HD inline float mcmc_sigmoid(float x) {
#pragma clang fp contract(off)
    return 1.f / (1.f + expf(-x));
}

// 0 for a dead row (o <= min_opacity; a NaN opacity is dead too), else clamp(floor(o * 2^32), 1, 2^32 - 1).  o * 2^32 is exact in float32.
FDGS_MCMC_HD inline uint32_t mcmc_weight(float x_o, float min_opacity) {
#pragma clang fp contract(off)
    const float o = mcmc_sigmoid(x_o);
    if (!(o > min_opacity)) return 0u;
    const float w = floorf(o * 4294967296.f);
    if (w < 1.f) return 1u;
    if (w >= 4294967296.f) return 0xFFFFFFFFu;
    return (uint32_t)w;
}

// the source of draw k: scan = inclusive uint64 sums of the weights, total = scan[N - 1] > 0
FDGS_MCMC_HD inline int mcmc_draw(int N, const uint64_t* scan, uint64_t total, uint32_t seed, uint32_t tag, uint32_t k) {
    uint32_t w[4];
    philox4x32_10(k, 0u, 0u, 0u, seed, tag, w);
    const uint64_t u = ((uint64_t)w[1] << 32) | w[0];
    const uint64_t r = mcmc_mulhi64(u, total);          // uniform on [0, total)
    int lo = 0, hi = N - 1;                              // first row whose inclusive sum exceeds r (exists: r < total = scan[N - 1])
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (scan[mid] > r) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// ---- relocation values --------------------------------------------------------------------------------------------------------------------
constexpr int MCMC_MAX_RATIO = FDGS_MCMC_MAX_RATIO;      // 51
struct McmcBinomials { double c[MCMC_MAX_RATIO + 1][MCMC_MAX_RATIO + 1]; };       // c[n][k] = C(n, k), exact in double up to C(51, 25) < 2^53
constexpr McmcBinomials mcmc_make_binomials() {
    McmcBinomials t{};
    for (int n = 0; n <= MCMC_MAX_RATIO; n++) {
        t.c[n][0] = 1.0;
        for (int k = 1; k <= n; k++) t.c[n][k] = t.c[n - 1][k - 1] + (k <= n - 1 ? t.c[n - 1][k] : 0.0);
    }
    return t;
}
#if defined(__HIPCC__)
__device__ __constant__ const McmcBinomials mcmc_binomials_dev = mcmc_make_binomials();
#endif
static const McmcBinomials mcmc_binomials_host = mcmc_make_binomials();
FDGS_MCMC_HD inline double mcmc_binomial(int n, int k) {
#if defined(__HIP_DEVICE_COMPILE__)
    return mcmc_binomials_dev.c[n][k];
#else
    return mcmc_binomials_host.c[n][k];
#endif
}

FDGS_MCMC_HD inline uint32_t mcmc_float_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
FDGS_MCMC_HD inline float mcmc_bits_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
// the next float32 towards +inf (finite, non-zero arguments)
FDGS_MCMC_HD inline float mcmc_next_up(float f) {
    const uint32_t u = mcmc_float_bits(f);
    return mcmc_bits_float((u >> 31) ? u - 1u : u + 1u);
}

// A source with raw opacity x_o and raw scales x_s[3], drawn `count` times: ratio r = min(count + 1, 51),
//   o' = 1 - (1 - o)^(1/r),  D = sum_{i=1..r} sum_{k=0..i-1} C(i-1,k) (-1)^k o'^(k+1) / sqrt(k+1),  s' = s o / D,
//   o' clamped to [min_opacity, 1 - 2^-23],  x_o' = log(o' / (1 - o')),  x_s' = log(s').
// Everything in double from the raw parameters: log(1 - o) = -softplus(x_o) and log(o) = -softplus(-x_o) without forming 1 - o,
// o' = -expm1(log(1 - o) / r) and 1 - o' = exp(log(1 - o) / r).  The inner sums of D are closed by sum_{i=k+1..r} C(i-1, k) = C(r, k+1):
//   D = sum_{k=0..r-1} (-1)^k C(r, k+1) o'^(k+1) / sqrt(k+1)          (the same number; r terms from row r of the binomial table).
// At r = 1: o' = o, D = o, and the float32 results are the inputs bit for bit (unless the clamp acts).
// Where the LOWER clamp acts, x_o' is not rounded to nearest but to the first float32 at least 3/4 of a unit above the double value (so
// between 0.75 and 1.75 units above it): the float32 expression of the dead test (mcmc_sigmoid(x_o') <= min_opacity, good to ~2.6 units
// of o, and one unit of x_o' near logit(0.005) is five units of o) must not call the row it has just been filled with dead.
FDGS_MCMC_HD inline void mcmc_relocation(float x_o, const float* x_s, uint32_t count, float min_opacity, float* x_o_new, float* x_s_new) {
#pragma clang fp contract(off)
    const int r = count >= (uint32_t)(MCMC_MAX_RATIO - 1) ? MCMC_MAX_RATIO : (int)count + 1;
    const double x = (double)x_o;
    const double lp = log1p(exp(-fabs(x)));
    const double log_1mo = -((x > 0.0 ? x : 0.0) + lp);          // log(1 - o)
    const double log_o = -((x < 0.0 ? -x : 0.0) + lp);           // log(o)
    const double log_q = log_1mo / (double)r;                    // log(1 - o')
    double on = -expm1(log_q);                                   // o'
    double D = 0.0, p = on;
    for (int k = 0; k < r; k++) {
        const double term = mcmc_binomial(r, k + 1) * p / sqrt((double)(k + 1));
        D = (k & 1) ? D - term : D + term;
        p = p * on;
    }
    const double dls = log_o - log(D);                           // log(s' / s)
    for (int c = 0; c < 3; c++) x_s_new[c] = (float)((double)x_s[c] + dls);
    const double lo = (double)min_opacity, hi = 1.0 - 1.1920928955078125e-07;
    double xo;
    bool low = false;
    if (on < lo) { xo = log(lo) - log1p(-lo); low = true; }
    else if (on > hi) xo = log(hi) - log(1.1920928955078125e-07);
    else xo = log(on) - log_q;
    float xf = (float)xo;
    if (low) {
        const double margin = 0.75 * ((double)mcmc_next_up(xf) - (double)xf);
        while ((double)xf < xo + margin) xf = mcmc_next_up(xf);
    }
    *x_o_new = xf;
}

// ---- noise --------------------------------------------------------------------------------------------------------------------------------
// Philox counter (row, iteration, 0, 0), key (seed, FDGS_MCMC_TAG_NOISE) -> words w0 .. w3;
//   (z0, z1) = sqrt(-2 ln u1) (cos, sin)(2 pi u2) with u1 = (w0 + 1) 2^-32 in (0, 1] (float32: never 0), u2 = (w1 >> 8) 2^-24 (exact);
//   z2 = the cosine branch of (w2, w3).  |z| <= sqrt(64 ln 2) = 6.66.
FDGS_MCMC_HD inline void mcmc_normals3(uint32_t seed, uint32_t row, uint32_t iteration, float* z) {
#pragma clang fp contract(off)
    uint32_t w[4];
    philox4x32_10(row, iteration, 0u, 0u, seed, (uint32_t)FDGS_MCMC_TAG_NOISE, w);
    const float ua = ((float)w[0] + 1.f) * 2.3283064365386963e-10f, ub = ((float)w[2] + 1.f) * 2.3283064365386963e-10f;
    const float ta = 6.283185307179586f * ((float)(w[1] >> 8) * 5.9604644775390625e-08f);
    const float tb = 6.283185307179586f * ((float)(w[3] >> 8) * 5.9604644775390625e-08f);
    const float la = -2.f * logf(ua), lb = -2.f * logf(ub);
    const float ra = sqrtf(la), rb = sqrtf(lb);
    z[0] = ra * cosf(ta);
    z[1] = ra * sinf(ta);
    z[2] = rb * cosf(tb);
}

// out = xyz + (R diag(s^2) R^T) xi * g * lr with s = exp(x_s), R = R(q / |q|) (gs_math.h: quat_to_R), o = sigmoid(x_o),
// g = 1 / (1 + exp(k_gate (o - min_opacity))).  out may alias xyz.
// Evaluated in DOUBLE from the float32 inputs, rounded once by the final add.  In float32 the entries of R carry an ABSOLUTE error of
// 2^-24 (1 - 2 (y^2 + z^2) next to 1), which a strongly anisotropic Gaussian multiplies by its largest s^2: the step then misses a bound
// relative to |M_ij| (measured: up to 3.1 x the test's bound at scale ratios of e^4).  A device kernel moves 56 bytes per row; ~60 double
// operations and five double exp / sqrt per row hide behind that (vector FP64 runs at the full rate on gfx950).
FDGS_MCMC_HD inline void mcmc_noise_row(const float* xyz, const float* x_s, const float* q, float x_o, const float* xi, float lr, float k_gate,
                                        float min_opacity, float* out) {
#pragma clang fp contract(off)
    const double o = 1.0 / (1.0 + exp(-(double)x_o));
    const double g = 1.0 / (1.0 + exp((double)k_gate * (o - (double)min_opacity)));
    const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    const double len = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    const double r = q0 / len, x = q1 / len, y = q2 / len, z = q3 / len;
    double R[9];
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - r * z);       R[2] = 2.0 * (x * z + r * y);
    R[3] = 2.0 * (x * y + r * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - r * x);
    R[6] = 2.0 * (x * z - r * y);       R[7] = 2.0 * (y * z + r * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
    const double e0 = xi[0], e1 = xi[1], e2 = xi[2];
    double t[3];
    for (int k = 0; k < 3; k++) {                        // t = diag(s^2) R^T xi
        const double s = exp((double)x_s[k]);
        t[k] = (s * s) * (R[k] * e0 + R[3 + k] * e1 + R[6 + k] * e2);
    }
    const double scale = g * (double)lr;
    for (int i = 0; i < 3; i++)                          // xyz + (R t) g lr
        out[i] = (float)((double)xyz[i] + (R[3 * i] * t[0] + R[3 * i + 1] * t[1] + R[3 * i + 2] * t[2]) * scale);
}

}  // namespace fdgs
