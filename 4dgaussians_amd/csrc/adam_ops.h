// adam_ops.h -- the per-element Adam update, once, for the device kernels of adam.hip and their host twin.
//
//     m = m + (g - m) * (1 - b1)                   (lerp)
//     v = b2 * v + (1 - b2) * g * g
//     p = p - step_size * m / (sqrt(v) / sqrt_bc2 + eps)
// step_size = lr / (1 - b1^t) and sqrt_bc2 = sqrt(1 - b2^t) with the bias corrections (torch's single-tensor Adam), lr and 1 without them
// (the sparse Adam kernels of graphdeco's rasterizer and gsplat); both are formed in double on the host (adam_scalars).
#pragma once
#include <math.h>

namespace fdgs {

struct AdamHyper {
    float b2, eps;
    float omb1, omb2;   // 1 - beta computed in double on the host like torch (1 - 0.999f in float is 2e-6 off)
};

__host__ __device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, float step_size, float sqrt_bc2, const AdamHyper& h) {
    m = m + (g - m) * h.omb1;
    v = h.b2 * v + h.omb2 * g * g;
    const float denom = sqrtf(v) / sqrt_bc2 + h.eps;
    p = p - step_size * (m / denom);
}

inline AdamHyper adam_hyper(double beta1, double beta2, double eps) {
    AdamHyper h;
    h.b2 = (float)beta2; h.eps = (float)eps;
    h.omb1 = (float)(1.0 - beta1); h.omb2 = (float)(1.0 - beta2);
    return h;
}

// the two per-tensor scalars of a tensor at step count t (after this step, t >= 1)
inline void adam_scalars(double lr, int t, double beta1, double beta2, bool bias_correction, float* step_size, float* sqrt_bc2) {
    if (bias_correction) {
        const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
        *step_size = (float)(lr / bc1);
        *sqrt_bc2 = (float)sqrt(bc2);
    } else {
        *step_size = (float)lr;
        *sqrt_bc2 = 1.0f;
    }
}

}  // namespace fdgs
