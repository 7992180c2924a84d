// adam.hip -- multi-tensor Adam step (one launch for up to 64 parameter tensors).
//
// Replaces `gaussians.optimizer.step()` (train.py:291) = torch.optim.Adam(l, lr=0.0, eps=1e-15) over the eight per-Gaussian
// groups plus the deformation MLP / HexPlane groups (scene/gaussian_model.py:165-196): betas (0.9, 0.999), no weight decay,
// no amsgrad, per-group lr set every iteration by update_learning_rate (:198-212).  Arithmetic follows torch's
// single-tensor Adam:
//     m = m + (g - m) * (1 - b1)                   (lerp)
//     v = b2 * v + (1 - b2) * g * g
//     p = p - (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// HBM-bound streaming kernel: 28 B per parameter element (p, m, v read+write, g read), float4 accesses, all tensors of a
// step in one launch (the per-tensor launch + ~5 elementwise passes of the foreach path cost more than the math at 200 fps).
//
// Sparse Adam (fdgs_adam_step_rows): the same launch with a per-tensor row mask.  A tensor is [rows, row_len]; a row whose mask byte is 0
// keeps its parameter and both moments bit for bit and its gradient is not looked at (graphdeco's SparseGaussianAdam, gsplat's
// SelectiveAdam).  One thread still owns one float4 of the four arrays: it finds the one to four rows its elements lie in, and when none of
// them is visible it issues no load and no store, so the HBM traffic follows the live rows (which cluster in the spatial order the library
// keeps).  Both walks are ONE kernel body around ONE adam1 (adam_ops.h): the dense instantiation is what fdgs_adam_step has always launched.
#include "common.h"
#include "adam_ops.h"

namespace fdgs {

constexpr int ADAM_MAX_TENSORS = 64;
struct AdamT {
    float* p; const float* g; float* m; float* v;
    unsigned int n;
    float step_size;      // lr / (1 - b1^t)
    float sqrt_bc2;       // sqrt(1 - b2^t)
    int first_block;
};
struct AdamArgs {
    AdamT t[ADAM_MAX_TENSORS];
    int ntensors;
    AdamHyper h;
};
// ... with a row mask.  64 tensors have to stay inside the 4 KB of kernel arguments: 56 bytes per tensor, the row lengths beside them
struct AdamRowsT {
    float* p; const float* g; float* m; float* v;
    const unsigned char* vis;   // [n / row_len] bytes, NULL: every row is stepped
    unsigned int n;
    float step_size, sqrt_bc2;
    int first_block;
};
struct AdamRowsArgs {
    AdamRowsT t[ADAM_MAX_TENSORS];
    unsigned int row_len[ADAM_MAX_TENSORS];
    int ntensors;
    AdamHyper h;
};
static_assert(sizeof(AdamRowsArgs) <= 4096, "kernel arguments");

// Bit k set: element e + k (k < cnt <= 4) lies in a visible row.  Reads vis[] only at the rows of those cnt elements.
__host__ __device__ __forceinline__ unsigned int rows_live(const unsigned char* vis, unsigned int row_len, unsigned int e, unsigned int cnt) {
    unsigned int r = e / row_len, rem = e - r * row_len, live = 0;
    bool on = cnt > 0 && vis[r] != 0;
    for (unsigned int k = 0; k < cnt; k++) {
        live |= (on ? 1u : 0u) << k;
        if (++rem == row_len && k + 1 < cnt) { rem = 0; on = vis[++r] != 0; }
    }
    return live;
}

template <bool ROWS, typename Args>
__global__ void __launch_bounds__(256) adam_kernel(Args a) {
    int lo = 0, hi = a.ntensors - 1;   // last tensor whose first_block <= blockIdx.x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.t[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const auto T = a.t[lo];
    const unsigned int e4 = ((unsigned int)blockIdx.x - (unsigned int)T.first_block) * 256u + threadIdx.x;
    const unsigned int n4 = T.n >> 2;
    unsigned int live = 0xFu;          // which of this thread's elements are stepped
    if constexpr (ROWS) {
        if (T.vis) {
            const unsigned int cnt = e4 < n4 ? 4u : e4 == n4 ? (T.n & 3u) : 0u;
            live = cnt ? rows_live(T.vis, a.row_len[lo], e4 * 4u, cnt) : 0u;
            if (live == 0) return;     // no load, no store: the rows of this float4 are all out of view
        }
    }
    if (e4 < n4) {
        float4 p = reinterpret_cast<float4*>(T.p)[e4], m = reinterpret_cast<float4*>(T.m)[e4], v = reinterpret_cast<float4*>(T.v)[e4];
        const float4 g = reinterpret_cast<const float4*>(T.g)[e4];
        if (!ROWS || live == 0xFu) {
            adam1(p.x, g.x, m.x, v.x, T.step_size, T.sqrt_bc2, a.h); adam1(p.y, g.y, m.y, v.y, T.step_size, T.sqrt_bc2, a.h);
            adam1(p.z, g.z, m.z, v.z, T.step_size, T.sqrt_bc2, a.h); adam1(p.w, g.w, m.w, v.w, T.step_size, T.sqrt_bc2, a.h);
        } else {                       // the other lanes' loaded bits go back unchanged: this thread owns the whole float4
            if (live & 1u) adam1(p.x, g.x, m.x, v.x, T.step_size, T.sqrt_bc2, a.h);
            if (live & 2u) adam1(p.y, g.y, m.y, v.y, T.step_size, T.sqrt_bc2, a.h);
            if (live & 4u) adam1(p.z, g.z, m.z, v.z, T.step_size, T.sqrt_bc2, a.h);
            if (live & 8u) adam1(p.w, g.w, m.w, v.w, T.step_size, T.sqrt_bc2, a.h);
        }
        reinterpret_cast<float4*>(T.p)[e4] = p; reinterpret_cast<float4*>(T.m)[e4] = m; reinterpret_cast<float4*>(T.v)[e4] = v;
    } else if (e4 == n4) {   // scalar tail (n % 4 elements) by one thread
        for (unsigned int i = n4 * 4; i < T.n; i++)
            if (!ROWS || ((live >> (i - n4 * 4)) & 1u)) adam1(T.p[i], T.g[i], T.m[i], T.v[i], T.step_size, T.sqrt_bc2, a.h);
    }
}

static int blocks_of(size_t n) { return cdiv((long long)(n / 4) + 1, 256); }

// what both fdgs_adam_step_rows and its host twin refuse
static int check_rows_tensor(const fdgs_adam_rows_tensor& s) {
    FDGS_REQUIRE(s.param && s.grad && s.exp_avg && s.exp_avg_sq, "adam: NULL tensor pointer");
    FDGS_REQUIRE(s.step >= 1, "adam: step counts from 1");
    FDGS_REQUIRE(s.row_len >= 1, "adam: row_len counts from 1");
    FDGS_REQUIRE(aligned_to(s.param, 16) && aligned_to(s.grad, 16) && aligned_to(s.exp_avg, 16) && aligned_to(s.exp_avg_sq, 16),
                 "adam: tensors must be 16-byte aligned");
    FDGS_REQUIRE(s.rows < (1ull << 32) && s.rows * (size_t)s.row_len < (1ull << 32), "adam: tensor too large");
    return FDGS_OK;
}

}  // namespace fdgs

using namespace fdgs;

extern "C" int fdgs_adam_step(void* stream_, int ntensors, const fdgs_adam_tensor* tensors, double beta1, double beta2, double eps) {
    FDGS_REQUIRE(ntensors >= 0 && (tensors || ntensors == 0), "bad tensor list");
    hipStream_t stream = (hipStream_t)stream_;
    int i = 0;   // next input tensor: empty tensors are skipped without using a slot, so the consumed index is tracked
    while (i < ntensors) {
        AdamArgs a{};
        int blocks = 0, cnt = 0;
        for (; i < ntensors && cnt < ADAM_MAX_TENSORS; i++) {
            const fdgs_adam_tensor& s = tensors[i];
            if (s.n == 0) continue;
            FDGS_REQUIRE(s.param && s.grad && s.exp_avg && s.exp_avg_sq, "adam: NULL tensor pointer");
            FDGS_REQUIRE(s.step >= 1, "adam: step counts from 1");
            FDGS_REQUIRE(aligned_to(s.param, 16) && aligned_to(s.grad, 16) && aligned_to(s.exp_avg, 16) && aligned_to(s.exp_avg_sq, 16),
                         "adam: tensors must be 16-byte aligned");
            FDGS_REQUIRE(s.n < (1ull << 32), "adam: tensor too large");
            AdamT& T = a.t[cnt++];
            T.p = s.param; T.g = s.grad; T.m = s.exp_avg; T.v = s.exp_avg_sq; T.n = (unsigned int)s.n;
            adam_scalars((double)s.lr, s.step, beta1, beta2, true, &T.step_size, &T.sqrt_bc2);
            T.first_block = blocks;
            blocks += blocks_of(s.n);
        }
        if (cnt == 0) continue;
        a.ntensors = cnt; a.h = adam_hyper(beta1, beta2, eps);
        { FDGS_TIMED("adam_step", stream); hipLaunchKernelGGL((adam_kernel<false, AdamArgs>), dim3(blocks), dim3(256), 0, stream, a); }
        FDGS_LAUNCH_CHECK("adam_step", 0, stream);
    }
    return FDGS_OK;
}

extern "C" int fdgs_adam_step_rows(void* stream_, int ntensors, const fdgs_adam_rows_tensor* tensors, double beta1, double beta2, double eps,
                                   int bias_correction) {
    FDGS_REQUIRE(ntensors >= 0 && (tensors || ntensors == 0), "bad tensor list");
    for (int k = 0; k < ntensors; k++)   // the whole list before the first launch: a refused call has stepped nothing
        if (tensors[k].rows != 0) { const int rc = check_rows_tensor(tensors[k]); if (rc != FDGS_OK) return rc; }
    hipStream_t stream = (hipStream_t)stream_;
    int i = 0;
    while (i < ntensors) {
        AdamRowsArgs a{};
        int blocks = 0, cnt = 0;
        for (; i < ntensors && cnt < ADAM_MAX_TENSORS; i++) {
            const fdgs_adam_rows_tensor& s = tensors[i];
            if (s.rows == 0) continue;
            const size_t n = s.rows * (size_t)s.row_len;
            a.row_len[cnt] = (unsigned int)s.row_len;
            AdamRowsT& T = a.t[cnt++];
            T.p = s.param; T.g = s.grad; T.m = s.exp_avg; T.v = s.exp_avg_sq; T.vis = s.visible; T.n = (unsigned int)n;
            adam_scalars((double)s.lr, s.step, beta1, beta2, bias_correction != 0, &T.step_size, &T.sqrt_bc2);
            T.first_block = blocks;
            blocks += blocks_of(n);
        }
        if (cnt == 0) continue;
        a.ntensors = cnt; a.h = adam_hyper(beta1, beta2, eps);
        { FDGS_TIMED("adam_step_rows", stream); hipLaunchKernelGGL((adam_kernel<true, AdamRowsArgs>), dim3(blocks), dim3(256), 0, stream, a); }
        FDGS_LAUNCH_CHECK("adam_step_rows", 0, stream);
    }
    return FDGS_OK;
}

// host twin (no GPU): the same walk in groups of four elements, rows_live and adam1 over host arrays
extern "C" int fdgs_adam_step_rows_host(int ntensors, const fdgs_adam_rows_tensor* tensors, double beta1, double beta2, double eps,
                                        int bias_correction) {
    FDGS_REQUIRE(ntensors >= 0 && (tensors || ntensors == 0), "bad tensor list");
    for (int k = 0; k < ntensors; k++)
        if (tensors[k].rows != 0) { const int rc = check_rows_tensor(tensors[k]); if (rc != FDGS_OK) return rc; }
    const AdamHyper h = adam_hyper(beta1, beta2, eps);
    for (int k = 0; k < ntensors; k++) {
        const fdgs_adam_rows_tensor& s = tensors[k];
        const size_t n = s.rows * (size_t)s.row_len;
        float step_size, sqrt_bc2;
        adam_scalars((double)s.lr, s.step, beta1, beta2, bias_correction != 0, &step_size, &sqrt_bc2);
        for (size_t e = 0; e < n; e += 4) {
            const unsigned int cnt = (unsigned int)(n - e < 4 ? n - e : 4);
            const unsigned int live = s.visible ? rows_live(s.visible, (unsigned int)s.row_len, (unsigned int)e, cnt) : 0xFu;
            for (unsigned int j = 0; j < cnt; j++)
                if ((live >> j) & 1u) adam1(s.param[e + j], s.grad[e + j], s.exp_avg[e + j], s.exp_avg_sq[e + j], step_size, sqrt_bc2, h);
        }
    }
    return FDGS_OK;
}
