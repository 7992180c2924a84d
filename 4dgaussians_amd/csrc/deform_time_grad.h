// deform_time_grad.h -- dL/dt of the deformation: the coordinate gradient of the three time planes, summed per row (per-Gaussian times) or
// over all rows (one frame time), with no float atomics anywhere.  Included by deform.hip inside namespace fdgs, after deform_plane_grad.h.
// Never on the default frame path: fdgs_deform_time_grad runs these kernels BEHIND a finished fdgs_deform_bwd, on the DFEAT rows that call's
// backward-data kernel (D2) left in the scratch; the plane-gradient kernels (D4), their launch plans and their registers are untouched.
//
// The time reaches the deformation only through the fourth HexPlane coordinate (scene/deformation.py: `timenet` is built, never called), so
//   dt_n = sum_lvl sum_c dfeat[n][lvl C + c] * sum_{k in {2,4,5}} (prod_{k' != k} v_k'[c]) * dscale_t * sum_x w_x (P_k[t1][x][c] - P_k[t0][x][c])
// with v_k the six bilinear samples of the level and (t0, t1, dscale_t) = axis_sample(t, res_t): exactly the `gy` D4 forms for bx == 3 and
// drops.  dscale_t = 0 where the border clamp is active: t at or beyond the last time row has a gradient of exactly 0.
//
//   deform_time_grad_partial_kernel<C>   lanes <-> (x-corner, channel) of one row as in D4's per-corner kernel, so every texel request is a
//       whole 64- / 128-byte line; 64 / (2 C) rows per wave step.  A workgroup owns TG_ROWS consecutive positions of what D2 walked -- the
//       live-row list (DFEAT indexed by list position, coordinates by the listed Gaussian, ROW_PAD entries dead) or, in the tile form, the
//       rows 0 .. N with `tile_live` deciding -- a fixed function of the position, no work stealing.  Dead rows are never read (a dead tile's
//       DFEAT rows are garbage): their DFEAT load is replaced by a select, and a wave step without a live row is skipped.  A lane adds its
//       3 L addends in (level, plane) order, the row's 2 C lanes are added by an xor butterfly (fixed order).
//         per-Gaussian times (p.time): dt_n is STORED to d_time[n] for every n < N (0 for dead rows): the caller never fills the array;
//         one frame time: a lane group adds its rows in ascending order, the workgroup's 4 * 64 / (2 C) group sums go through LDS and are added
//         by one thread in index order: one float per workgroup into `partials` (a workgroup behind the list's end stores 0).
//   deform_time_grad_final_kernel        one workgroup: thread i adds partials i, i + 256, ... in double, then a fixed tree over the 256 doubles
//       in LDS, one float out.  For given DFEAT rows the result is the same bits on every run.
//   deform_time_grad_dfeat_kernel        the probe: DFEAT of the live rows -> Gaussian order [N][C L] + one live byte per row (plain vector
//       stores; tests feed the host twin with the kernel's own input).
constexpr int TG_ROWS = 256;          // positions per workgroup of the partial kernel
struct TimeGradArgs {
    fdgs_deform_params p;
    AabbScale sc;
    const float* DFEAT;
    const uint32_t* tile_live;        // tile form: [Npad/32], != 0 = D2 wrote the tile's DFEAT rows
    const uint32_t* rows;             // row-list form (non-NULL): the live-row list, counters[5] * 32 entries
    const uint32_t* counters;
    int F;
    float* d_time;                    // per-Gaussian times: [N]; NULL with one frame time
    float* partials;                  // one frame time: [gridDim.x]
};

template <int C>
__global__ void __launch_bounds__(256) deform_time_grad_partial_kernel(TimeGradArgs a) {
    const fdgs_deform_params& p = a.p;
    constexpr int LPG = 2 * C, GPW = 64 / LPG, NGRP = 4 * GPW;
    __shared__ float s_grp[NGRP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ch = lane % C, xc = (lane / C) & 1, gsub = lane / LPG;
    const bool by_rows = a.rows != nullptr;
    const int total = by_rows ? (int)as_const(a.counters)[5] * 32 : p.N;
    const int e_begin = blockIdx.x * TG_ROWS;
    float run = 0.f;
    for (int it = 0; it < TG_ROWS / NGRP; it++) {
        const int e = e_begin + it * NGRP + wave * GPW + gsub;
        bool live = e < total;
        int n = 0;
        if (live) {
            if (by_rows) {
                const uint32_t ent = a.rows[e];
                live = !(ent & ROW_PAD);
                n = (int)(ent & ~ROW_PAD);
            } else {
                n = e;
                live = a.tile_live[e >> 5] != 0u;
            }
        }
        if (__ballot(live) == 0ull) {       // (wave-uniform) nothing to read; per-Gaussian times still get their zeros
            if (a.d_time && (lane % LPG) == 0 && e < total) a.d_time[e] = 0.f;
            continue;
        }
        if (!live) n = 0;                   // (a valid row to take coordinates from; its DFEAT row is not read)
        float q[4];
#pragma unroll
        for (int i = 0; i < 3; i++) q[i] = query_coord(p.xyz[3 * (size_t)n + i], p.aabb[i], a.sc.inv2[i]);
        q[3] = p.time ? p.time[n] : p.time_scalar;
        float acc = 0.f;
        for (int lvl = 0; lvl < p.L; lvl++) {
            const float df = live ? a.DFEAT[(size_t)(by_rows ? e : n) * a.F + lvl * C + ch] : 0.f;
            AxisSample S[4];
#pragma unroll
            for (int ax4 = 0; ax4 < 4; ax4++) S[ax4] = axis_sample(q[ax4], p.res[lvl][ax4]);
            float vk[6], tk[6];
#pragma unroll
            for (int k = 0; k < 6; k++) {
                int ax, bx;
                plane_axes(k, ax, bx);
                const int Wd = p.res[lvl][ax];
                const AxisSample sx = S[ax], sy = S[bx];
                const int xi = xc ? sx.i1 : sx.i0;
                const float wx = xc ? sx.w1 : sx.w0;
                const uint32_t oA = (uint32_t)((sy.i0 * Wd + xi) * C + ch), oB = (uint32_t)((sy.i1 * Wd + xi) * C + ch);
                const char* Pb = reinterpret_cast<const char*>(p.planes[lvl][k]);   // SGPR base + 32-bit byte offset
                const float v0 = *reinterpret_cast<const float*>(Pb + oA * 4u);
                const float v1 = *reinterpret_cast<const float*>(Pb + oB * 4u);
                const float part = wx * (sy.w0 * v0 + sy.w1 * v1);
                vk[k] = part + __shfl_xor(part, C, 64);       // both x-corners
                tk[k] = wx * (v1 - v0);                       // d/d(iy); used for the time planes only
            }
            float pre[6], suf[6];
            pre[0] = 1.f; suf[5] = 1.f;
#pragma unroll
            for (int k = 1; k < 6; k++) pre[k] = pre[k - 1] * vk[k - 1];
#pragma unroll
            for (int k = 4; k >= 0; k--) suf[k] = suf[k + 1] * vk[k + 1];
#pragma unroll
            for (int k = 0; k < 6; k++)
                if (time_plane_slot(k) >= 0) acc += (df * pre[k] * suf[k]) * tk[k] * S[3].dscale;
        }
#pragma unroll
        for (int o = 1; o < LPG; o <<= 1) acc += __shfl_xor(acc, o, 64);
        const float dt = live ? acc : 0.f;
        if (a.d_time) {
            if ((lane % LPG) == 0 && e < total) a.d_time[e] = dt;      // (per-Gaussian times: always the tile form, e is the Gaussian)
        } else {
            run += dt;
        }
    }
    if (a.d_time) return;
    if ((lane % LPG) == 0) s_grp[wave * GPW + gsub] = run;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = s_grp[0];
#pragma unroll
        for (int i = 1; i < NGRP; i++) s += s_grp[i];
        a.partials[blockIdx.x] = s;
    }
}

__global__ void __launch_bounds__(256) deform_time_grad_final_kernel(const float* partials, int n, float* out) {
    __shared__ double s[256];
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) v += (double)partials[i];
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)s[0];
}

struct TimeGradProbeArgs {
    const float* DFEAT; const uint32_t* tile_live; const uint32_t* rows; const uint32_t* counters;
    int N, F;
    float* dfeat;       // [N][F], zero-filled by the caller
    uint8_t* live;      // [N], zero-filled by the caller
};
// one thread per (position, four channels); never on the frame path
__global__ void __launch_bounds__(256) deform_time_grad_dfeat_kernel(TimeGradProbeArgs a) {
    const int f4 = a.F / 4;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long e = idx / f4;
    const int j = (int)(idx - e * f4);
    const long long total = a.rows ? (long long)a.counters[5] * 32 : (long long)a.N;
    if (e >= total) return;
    long long n = e;
    if (a.rows) {
        const uint32_t ent = a.rows[e];
        if (ent & ROW_PAD) return;
        n = (long long)ent;
    } else if (a.tile_live[e >> 5] == 0u) {
        return;
    }
    reinterpret_cast<float4*>(a.dfeat + (size_t)n * a.F)[j] = reinterpret_cast<const float4*>(a.DFEAT + (size_t)e * a.F)[j];
    if (j == 0) a.live[n] = 1;
}

// The host twin (fdgs_deform_time_grad_host): the same helpers for the index arithmetic, every sum in double.  addend(lvl, k, x, c) =
// dfeat * prod_{k' != k} v_k' * dscale_t * w_x * (P_k[t1][x][c] - P_k[t0][x][c]); returns the row's sum and the sum of |addend|.
static void time_grad_row_host(const fdgs_deform_params& p, const float* inv2, size_t n, const float* dfeat_row, double* sum, double* abs_sum) {
    float q[4];
    for (int i = 0; i < 3; i++) q[i] = query_coord(p.xyz[3 * n + i], p.aabb[i], inv2[i]);
    q[3] = p.time ? p.time[n] : p.time_scalar;
    double s = 0.0, sa = 0.0;
    for (int lvl = 0; lvl < p.L; lvl++) {
        AxisSample S[4];
        for (int ax = 0; ax < 4; ax++) S[ax] = axis_sample(q[ax], p.res[lvl][ax]);
        for (int c = 0; c < p.C; c++) {
            double v[6];
            for (int k = 0; k < 6; k++) {
                int ax, bx;
                plane_axes(k, ax, bx);
                const int Wd = p.res[lvl][ax];
                const float* P = reinterpret_cast<const float*>(p.planes[lvl][k]);
                const AxisSample sx = S[ax], sy = S[bx];
                auto at = [&](int y, int x) { return (double)P[((size_t)y * Wd + x) * p.C + c]; };
                v[k] = (double)sx.w0 * ((double)sy.w0 * at(sy.i0, sx.i0) + (double)sy.w1 * at(sy.i1, sx.i0)) +
                       (double)sx.w1 * ((double)sy.w0 * at(sy.i0, sx.i1) + (double)sy.w1 * at(sy.i1, sx.i1));
            }
            const double df = (double)dfeat_row[lvl * p.C + c];
            for (int k = 0; k < 6; k++) {
                if (time_plane_slot(k) < 0) continue;
                double others = 1.0;
                for (int k2 = 0; k2 < 6; k2++) if (k2 != k) others *= v[k2];
                int ax, bx;
                plane_axes(k, ax, bx);
                const int Wd = p.res[lvl][ax];
                const float* P = reinterpret_cast<const float*>(p.planes[lvl][k]);
                const AxisSample sx = S[ax], st = S[3];
                for (int x = 0; x < 2; x++) {
                    const int xi = x ? sx.i1 : sx.i0;
                    const double wx = x ? (double)sx.w1 : (double)sx.w0;
                    const double d = (double)P[((size_t)st.i1 * Wd + xi) * p.C + c] - (double)P[((size_t)st.i0 * Wd + xi) * p.C + c];
                    const double addend = df * others * (double)st.dscale * wx * d;
                    s += addend;
                    sa += fabs(addend);
                }
            }
        }
    }
    *sum = s;
    *abs_sum = sa;
}
