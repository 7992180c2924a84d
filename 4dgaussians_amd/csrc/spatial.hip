// spatial.hip -- the spatial order of the Gaussian set: space-filling-curve keys of the positions and their STABLE argsort.
//
// What a caller of fdgs_permute_rows needs to produce its permutation: the Hilbert (or Morton) key of every position (spatial_keys.h: the
// torch expressions of fdgs.densify restated bit for bit), the bounding box when no bounds are given, and an LSD radix sort of (key, row
// index) pairs over the 3 * bits key bits -- binning.hip's radix_sort_pairs as it is.  Every pass is stable and the payload starts as
// 0 .. N-1, so the sorted payload is THE stable ascending argsort (ties keep their row order), not merely a valid one.
//
// Launches per fdgs_spatial_order: [bbox partials + bbox final when bounds are NULL] + keys + 3 x ceil(3 * bits / 8) radix launches (30 bits:
// digit widths 8, 8, 7, 7), all on the caller's stream, no synchronisation, no read-back.
#include "common.h"
#include "raster.h"
#include "spatial_keys.h"

namespace fdgs {

constexpr int BBOX_MAX_BLOCKS = 256;                 // partial boxes (one per workgroup of the first reduction launch)
constexpr int BBOX_POINTS_PER_BLOCK = 256 * 16;
// sets up to this size sort in 1024-key workgroups (what the depth sort of the Gaussians uses: at 300 k keys 4096-key workgroups are 74 on
// 256 CUs), larger ones in 4096-key workgroups (the digit scan then stays one 1024-counter round per digit up to 4 M keys)
constexpr int SPATIAL_SMALL_SORT_MAX = 1 << 20;

struct SpatialScratch {
    size_t bounds, partial, keys0, keys1, vals, hist, bytes;
    int items, sort_blocks;
};
inline SpatialScratch spatial_scratch(int N) {
    SpatialScratch s{};
    size_t o = 0;
    const size_t n = (size_t)(N > 0 ? N : 1);
    auto take = [&](size_t bytes) { size_t r = o; o = align_up(o + bytes); return r; };
    s.bounds = take(6 * sizeof(float));                                   // lo[3], hi[3] of the bounding box
    s.partial = take((size_t)BBOX_MAX_BLOCKS * 6 * sizeof(float));
    s.keys0 = take(n * 4);
    s.keys1 = take(n * 4);
    s.vals = take(n * 4);
    s.items = N <= SPATIAL_SMALL_SORT_MAX ? NSORT_ITEMS : SORT_ITEMS;
    s.sort_blocks = cdiv((long long)n, SORT_THREADS * s.items);
    // (sized for the 1024-key form at every N, so that the size grows monotonically across the switch of the workgroup size)
    s.hist = take(((size_t)RADIX * cdiv((long long)n, NSORT_CHUNK) + 1024) * 4);
    s.bytes = o;
    return s;
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }

// Bounding box, launch 1: workgroup b reduces its grid-strided share of the points to partial[b][6] = { min xyz, max xyz }.  min / max are
// exact in any order; non-finite coordinates are left out (they are quantised to cell 0 whatever the box is).
__global__ void __launch_bounds__(256) spatial_bbox_partial_kernel(int N, const float* __restrict__ xyz, float* __restrict__ partial) {
    __shared__ float red[4][6];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float v = xyz[3 * i + c];
            if (finite_f(v)) { lo[c] = fminf(lo[c], v); hi[c] = fmaxf(hi[c], v); }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo[c] = fminf(lo[c], __shfl_xor(lo[c], o, 64));
            hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o, 64));
        }
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) { red[w][c] = lo[c]; red[w][3 + c] = hi[c]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int c = threadIdx.x;
        float v = red[0][c];
        for (int k = 1; k < 4; k++) v = c < 3 ? fminf(v, red[k][c]) : fmaxf(v, red[k][c]);
        partial[blockIdx.x * 6 + c] = v;
    }
}
// launch 2 (one workgroup): the partial boxes to bounds[6] = { min xyz, max xyz }
__global__ void __launch_bounds__(256) spatial_bbox_final_kernel(int nparts, const float* __restrict__ partial, float* __restrict__ bounds) {
    __shared__ float red[4][6];
    float v[6];
#pragma unroll
    for (int c = 0; c < 6; c++) v[c] = (int)threadIdx.x < nparts ? partial[threadIdx.x * 6 + c] : (c < 3 ? INFINITY : -INFINITY);
#pragma unroll
    for (int c = 0; c < 6; c++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float u = __shfl_xor(v[c], o, 64);
            v[c] = c < 3 ? fminf(v[c], u) : fmaxf(v[c], u);
        }
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 6; c++) red[w][c] = v[c];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int c = threadIdx.x;
        float r = red[0][c];
        for (int k = 1; k < 4; k++) r = c < 3 ? fminf(r, red[k][c]) : fmaxf(r, red[k][c]);
        bounds[c] = r;
    }
}

// keys[i] = curve key of row i, payload[i] = i (payload may be NULL)
__global__ void __launch_bounds__(256) spatial_keys_kernel(int N, const float* __restrict__ xyz, const float* __restrict__ bounds, int curve, int bits,
                                                           uint32_t* __restrict__ keys, uint32_t* __restrict__ payload) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    float b[6];
#pragma unroll
    for (int c = 0; c < 6; c++) b[c] = bounds[c];
    keys[i] = curve_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], b, curve, bits);
    if (payload) payload[i] = (uint32_t)i;
}

static int check_args(int N, const float* xyz, int curve, int bits, const void* scratch, bool need_scratch, const void* out) {
    FDGS_REQUIRE(N >= 0, "bad N (negative)");
    FDGS_REQUIRE(bits >= 1 && bits <= 10, "bad bits (1 .. 10)");
    FDGS_REQUIRE(curve == FDGS_CURVE_HILBERT || curve == FDGS_CURVE_MORTON, "bad curve (FDGS_CURVE_HILBERT | FDGS_CURVE_MORTON)");
    if (N == 0) return FDGS_OK;
    FDGS_REQUIRE(xyz && out && (scratch || !need_scratch), "NULL pointer");
    return FDGS_OK;
}

// keys (+ payload) of the N points on `stream`; the box comes from bounds_opt or is reduced into the scratch first
static int launch_keys(hipStream_t stream, int N, const float* xyz, const float* bounds_opt, int curve, int bits, void* scratch,
                       uint32_t* keys, uint32_t* payload) {
    const SpatialScratch s = spatial_scratch(N);
    const float* bounds = bounds_opt;
    if (!bounds) {
        float* box = at<float>(scratch, s.bounds);
        float* partial = at<float>(scratch, s.partial);
        int nparts = cdiv(N, BBOX_POINTS_PER_BLOCK);
        if (nparts > BBOX_MAX_BLOCKS) nparts = BBOX_MAX_BLOCKS;
        { FDGS_TIMED("spatial_bbox", stream);
          hipLaunchKernelGGL(spatial_bbox_partial_kernel, dim3(nparts), dim3(256), 0, stream, N, xyz, partial);
          hipLaunchKernelGGL(spatial_bbox_final_kernel, dim3(1), dim3(256), 0, stream, nparts, partial, box); }
        FDGS_LAUNCH_CHECK("spatial_bbox", 0, stream);
        bounds = box;
    }
    { FDGS_TIMED("spatial_keys", stream);
      hipLaunchKernelGGL(spatial_keys_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, N, xyz, bounds, curve, bits, keys, payload); }
    FDGS_LAUNCH_CHECK("spatial_keys", 0, stream);
    return FDGS_OK;
}
}  // namespace fdgs

using namespace fdgs;

extern "C" int fdgs_spatial_order_scratch_bytes(int N, size_t* bytes) {
    FDGS_REQUIRE(N >= 0 && bytes, "bad arguments");
    *bytes = spatial_scratch(N).bytes;
    return FDGS_OK;
}

extern "C" int fdgs_spatial_keys(void* stream_, int N, const float* xyz, const float* bounds_opt, int curve, int bits, void* scratch,
                                 uint32_t* keys) {
    // (with bounds given nothing is written to the scratch: it may then be NULL)
    const int rc = check_args(N, xyz, curve, bits, scratch, bounds_opt == nullptr, keys);
    if (rc != FDGS_OK || N == 0) return rc;
    return launch_keys((hipStream_t)stream_, N, xyz, bounds_opt, curve, bits, scratch, keys, nullptr);
}

extern "C" int fdgs_spatial_order(void* stream_, int N, const float* xyz, const float* bounds_opt, int curve, int bits, void* scratch,
                                  int32_t* perm, uint32_t* sorted_keys_opt) {
    int rc = check_args(N, xyz, curve, bits, scratch, true, perm);
    if (rc != FDGS_OK || N == 0) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const SpatialScratch s = spatial_scratch(N);
    // the sort ping-pongs between (k0, v0) and (k1, v1) and ends in pair (passes & 1): the caller's arrays take that pair's place
    const int nbits = 3 * bits, npass = (nbits + RADIX_BITS - 1) / RADIX_BITS, last = npass & 1;
    uint32_t* k[2] = {at<uint32_t>(scratch, s.keys0), at<uint32_t>(scratch, s.keys1)};
    uint32_t* v[2] = {at<uint32_t>(scratch, s.vals), at<uint32_t>(scratch, s.vals)};
    v[last] = reinterpret_cast<uint32_t*>(perm);
    if (sorted_keys_opt) k[last] = sorted_keys_opt;
    rc = launch_keys(stream, N, xyz, bounds_opt, curve, bits, scratch, k[0], v[0]);
    if (rc != FDGS_OK) return rc;
    int where = 0;
    rc = radix_sort_pairs(stream, k[0], v[0], k[1], v[1], (uint32_t)N, nbits, at<uint32_t>(scratch, s.hist), s.sort_blocks, 0, &where, s.items,
                          nullptr);
    if (rc != FDGS_OK) return rc;
    if (where != last) return fail(FDGS_E_INVALID, "%s", "spatial order: the sort ended in the other buffer pair");
    return FDGS_OK;
}

extern "C" int fdgs_spatial_keys_host(int N, const float* xyz, const float* bounds_opt, int curve, int bits, uint32_t* keys) {
    const int rc = check_args(N, xyz, curve, bits, nullptr, false, keys);
    if (rc != FDGS_OK || N == 0) return rc;
    float box[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    if (bounds_opt) {
        for (int c = 0; c < 6; c++) box[c] = bounds_opt[c];
    } else {
        for (size_t i = 0; i < (size_t)N; i++)
            for (int c = 0; c < 3; c++) {
                const float p = xyz[3 * i + c];
                if (fabsf(p) <= 3.402823466e38f) { box[c] = fminf(box[c], p); box[3 + c] = fmaxf(box[3 + c], p); }
            }
    }
    for (size_t i = 0; i < (size_t)N; i++) keys[i] = curve_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], box, curve, bits);
    return FDGS_OK;
}
