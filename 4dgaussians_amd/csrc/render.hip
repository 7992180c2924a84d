// render.hip -- K6 (front-to-back alpha blending) and K7 (its backward) for gfx950.
//
// Forward: one 256-thread workgroup (4 wave64) per 16x16-pixel tile, one pixel per lane; per round the workgroup stages 256 list
// entries (3 x float4 per Gaussian) in LDS and the inner loop reads them with wave-uniform (broadcast) ds_read_b128.
// Backward (round 3): ONE wave per tile, four pixels per lane as two packed-f32 pairs (render_bwd_strip_kernel): each lane recomputes
// alpha back-to-front, forms the per-Gaussian sums of its pixels as moments over dy, the wave adds them with a DPP / permlane
// reduce-scatter and issues ONE 64-byte atomic line-op per (tile, Gaussian) into a packed [P,16] gradient array.  The 256-thread
// backward of rounds 1-2 (four waves meeting in LDS slots) stays selectable (tuning knob rbwd_ppl = 0; 2 = two waves per tile with two
// pixels per lane): the three forms are compared with each other in tests/test_gpu_raster.py.  (A strip form of the FORWARD measured
// slower and was dropped in round 3.)  All three forms have an ABS instantiation (fdgs_raster_bwd_abs): beside the signed sums it adds, per
// Gaussian, the ABSOLUTE values of every pixel's screen-space gradient (the densification statistic of AbsGS) into slots 10 and 11 of the same
// line, with the same reductions and the same atomic; a frame that does not ask launches the instantiations it always launched.
// Pick pass (render_pick_kernel): the forward's layout once more over a finished frame's lists, for the id of the Gaussian with the largest
// blend weight and the id and depth of the one at which the accumulated alpha reaches a cut; it writes nothing into the frame.
// Contribution pass (render_contrib_kernel): that walk again, reduced per Gaussian instead of per pixel -- the sum and the maximum of the
// blend weight over the pixels, the pixels and the tiles that show it --, one atomic record per (tile, entry); it writes nothing into the frame.
// Feature pass (render_features_kernel): that walk with C per-row channels in place of the colour, sixteen per workgroup and all C in one launch,
// each with the bits a forward blend of it would give; it writes nothing into the frame.
// Feature pass backward (render_features_bwd_kernel, render_features_bwd.h): that walk once more for the gradient of the features to the values,
// the sum over a tile's pixels as a contraction on the matrix cores, one atomic per (tile, entry, channel); it writes nothing into the frame.
// Tile rows are dealt to the XCDs in groups (unit_of_block: workgroup b runs on XCD b % 8), so that neighbouring tiles -- which list
// the same Gaussians -- share an XCD's 4 MiB L2 and every XCD owns rows from the whole height of the image.
// Replaces renderCUDA forward/backward of the un-vendored rasterizer (Appendix B.3/B.4).
#include "common.h"
#include "gs_math.h"
#include "raster.h"
#include "tile_walk.h"

namespace fdgs {

// Workgroup b runs on XCD b % 8 (round-robin dispatch).  The tile rows are dealt to the XCDs in groups of `bh` rows: group G (rows
// G*bh .. G*bh+bh-1) belongs to XCD G % 8, and an XCD walks its groups top to bottom.  Neighbouring tiles (which list the same Gaussians)
// share an XCD's L2 inside a group, and every XCD owns rows from the whole height of the image: with ONE contiguous band per XCD (rounds
// 1-2) the bands that only see the rim of the scene ran empty while the XCDs of the central bands carried the frame.
// `parts` work units per tile (strip kernels: waves per tile), units of a tile adjacent.  Returns the unit index or -1.
__device__ __forceinline__ int unit_of_block(int b, int gx, int gy, int parts, int bh) {
    const int xcd = b & 7, idx = b >> 3;
    const int per_group = bh * gx * parts;
    const int g = idx / per_group, rem = idx - g * per_group;
    const int row = (g * 8 + xcd) * bh + rem / (gx * parts);
    if (row >= gy) return -1;
    return row * gx * parts + rem % (gx * parts);
}
__host__ __device__ __forceinline__ int unit_grid(int gx, int gy, int parts, int bh) {
    const int groups = (gy + bh - 1) / bh;
    return 8 * ((groups + 7) / 8) * bh * gx * parts;
}
// Heaviest-first dispatch (round 5).  A blending kernel is ONE wave (backward) or one workgroup (forward) per tile, the tiles' list
// lengths differ by 5x between the rim and the centre of the image, and with 5 440 tiles on 1 024 SIMDs x 4 wave slots nearly every
// tile is resident from the start: nothing balances the load, a SIMD that drew four centre tiles finishes long after one that drew
// four rim tiles (a dispatch simulation on the bench frame's per-tile work puts the backward at 0.62 of perfect balance in image order
// and at 0.82 heaviest-first; tools/tile_balance_sim.py).  `order` (tile_order_kernel) lists each XCD's tiles by descending work: block b
// still runs on XCD b % 8 and still only takes tiles of that XCD's row groups (their Gaussians stay in its L2), but the heavy ones are
// dispatched first and the light ones fill in behind them.  order == nullptr: image order.
__device__ __forceinline__ int unit_lookup(const uint32_t* __restrict__ order, int per_xcd, int b, int gx, int gy, int parts, int bh) {
    if (!order) return unit_of_block(b, gx, gy, parts, bh);
    const int xcd = b & 7, idx = b >> 3;
    const uint32_t t = order[xcd * per_xcd + idx / parts];
    return t == 0xFFFFFFFFu ? -1 : (int)t * parts + idx % parts;
}
// One 1024-thread workgroup per XCD: counting sort of the XCD's tiles by descending key (256 levels of the XCD's largest key; LPT needs
// no finer order), key = list length (mode 0, forward) or the forward's per-tile `todo` (mode 1, backward).  Padding slots of the map
// (rows below the image) and tiles with key 0 go last.
// (the body: XCD x's list from key_of(tile), by the 1024 threads of one workgroup; hist, base [256] and smax in LDS)
template <typename KeyF>
__device__ __forceinline__ void tile_order_body(uint32_t* hist, uint32_t* base, uint32_t& smax, int x, int gx, int gy, int bh, int per_xcd,
                                                uint32_t* __restrict__ order, KeyF key_of) {
    const int t = threadIdx.x;
    if (t < 256) hist[t] = 0;
    if (t == 0) smax = 0;
    __syncthreads();
    constexpr int PER = TILE_ORDER_MAX / 1024;
    int tile[PER];
    uint32_t key[PER];
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < PER; i++) {
        const int idx = t + 1024 * i;
        tile[i] = idx < per_xcd ? unit_of_block(idx * 8 + x, gx, gy, 1, bh) : -2;      // -1: padding slot of the map, -2: beyond the map
        key[i] = 0;
        if (tile[i] >= 0) key[i] = key_of(tile[i]);
        m = key[i] > m ? key[i] : m;
    }
    if (m) atomicMax(&smax, m);
    __syncthreads();
    const float scale = 255.0f / (float)(smax > 0 ? smax : 1u);
    uint32_t bucket[PER];
#pragma unroll
    for (int i = 0; i < PER; i++) {
        const uint32_t lvl = (uint32_t)((float)key[i] * scale);         // (monotonic in the key: all the order needs)
        bucket[i] = 255u - (lvl < 255u ? lvl : 255u);
        if (tile[i] == -1) bucket[i] = 255u;
        if (tile[i] != -2) atomicAdd(&hist[bucket[i]], 1u);
    }
    __syncthreads();
    if (t < 64) {       // exclusive scan of the 256 counts by one wave: four per lane
        const uint32_t c0 = hist[4 * t], c1 = hist[4 * t + 1], c2 = hist[4 * t + 2], c3 = hist[4 * t + 3];
        uint32_t inc = c0 + c1 + c2 + c3;
        const uint32_t tot = inc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(inc, o, 64); if (t >= o) inc += u; }
        const uint32_t ex = inc - tot;
        base[4 * t] = ex; base[4 * t + 1] = ex + c0; base[4 * t + 2] = ex + c0 + c1; base[4 * t + 3] = ex + c0 + c1 + c2;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PER; i++)
        if (tile[i] != -2) order[(size_t)x * per_xcd + atomicAdd(&base[bucket[i]], 1u)] = tile[i] >= 0 ? (uint32_t)tile[i] : 0xFFFFFFFFu;
}
__global__ void __launch_bounds__(1024) tile_order_kernel(int mode, int gx, int gy, int bh, int per_xcd, const uint2* __restrict__ ranges,
                                                          const uint32_t* __restrict__ todo, uint32_t* __restrict__ order) {
    __shared__ uint32_t hist[256], base[256], smax;
    tile_order_body(hist, base, smax, blockIdx.x, gx, gy, bh, per_xcd, order,
                    [&](int tile) -> uint32_t { return mode == 0 ? ranges[tile].y - ranges[tile].x : todo[tile]; });
}
// The scan of the tiles' pair counts into their ranges and the forward's tile order in ONE grid (the chain of a frame whose projection
// counted, binning.hip): both need nothing but the counts -- the order's key is the tile's list length, and that IS its count (a tile
// whose list the capacity mode drops keeps its count as the key: the order only decides dispatch).  Workgroups 0..7: the XCDs' orders
// (none when per_xcd == 0), the last workgroup: the scan.
__global__ void __launch_bounds__(1024) tile_scan_order_kernel(const uint32_t* __restrict__ cnt, uint32_t ntiles, uint2* __restrict__ ranges, uint32_t cap,
                                                               int gx, int gy, int bh, int per_xcd, uint32_t* __restrict__ order) {
    __shared__ uint32_t hist[256], base[256], smax, wsum[16];
    if (blockIdx.x == gridDim.x - 1) tile_scan_body(wsum, cnt, ntiles, ranges, nullptr, cap);
    else tile_order_body(hist, base, smax, blockIdx.x, gx, gy, bh, per_xcd, order, [&](int tile) -> uint32_t { return cnt[tile]; });
}

// The exponent of a blended Gaussian, written so that EVERY kernel that evaluates it rounds it the same way (the forward decides
// alpha >= 1/255 and T < 1e-4 from it, the backward has to take the same decisions): -0.5 * (dx*(dx*cxx) + dy*(dy*cyy)) - dy*(dx*cxy),
// products and the sum rounded separately, one fused multiply-add at the end.
__device__ __forceinline__ float blend_power_xx(float cxx, float dx) {
#pragma clang fp contract(off)
    return dx * (dx * cxx);
}
__device__ __forceinline__ float blend_power_xy(float cxy, float dx) {
#pragma clang fp contract(off)
    return dx * cxy;
}
__device__ __forceinline__ float blend_power(float u1, float cx, float cyy, float dy) {
#pragma clang fp contract(off)
    const float u2 = dy * (dy * cyy);
    const float c2 = dy * cx;
    const float q = u1 + u2;
    return __builtin_fmaf(q, -0.5f, -c2);
}
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2f blend_power2(float u1, float cx, float cyy, v2f dy) {
#pragma clang fp contract(off)
    const v2f u2 = dy * (dy * cyy);
    const v2f c2 = dy * cx;
    const v2f q = u1 + u2;
    return __builtin_elementwise_fma(q, v2f{-0.5f, -0.5f}, -c2);
}
// ... and element-wise for TWO Gaussians at one pixel (render_fwd_kernel<1>: the entries j and j + 1 of a list): per element the operations
// of blend_power_xx / blend_power_xy / blend_power, in their order
__device__ __forceinline__ v2f blend_power_xx_e2(v2f cxx, v2f dx) {
#pragma clang fp contract(off)
    return dx * (dx * cxx);
}
__device__ __forceinline__ v2f blend_power_xy_e2(v2f cxy, v2f dx) {
#pragma clang fp contract(off)
    return dx * cxy;
}
__device__ __forceinline__ v2f blend_power_e2(v2f u1, v2f cx, v2f cyy, v2f dy) {
#pragma clang fp contract(off)
    const v2f u2 = dy * (dy * cyy);
    const v2f c2 = dy * cx;
    const v2f q = u1 + u2;
    return __builtin_elementwise_fma(q, v2f{-0.5f, -0.5f}, -c2);
}

// what both blending kernels take first: the image's tile grid and the block -> tile map
struct BlendHead {
    int W, H, gx, gy, bh;
    const uint32_t* order; int per_xcd;      // heaviest-first tile order (nullptr: image order)
};

struct RenderArgs : BlendHead {
    uint32_t* tile_todo;                     // out, per tile: max n_contrib = the entries the backward will walk
    const uint2* ranges; const uint32_t* pair_gid;
    const float4 *recA, *recB, *recC;
    const float* bg;
    float* final_T; uint32_t* n_contrib;
    float *out_color, *out_depth;
    float* out_alpha;                        // opt [H*W]: the accumulated opacity 1 - final_T (fdgs_render_fwd_alpha)
    float4* zfill; uint32_t zfill_n4;        // opt: a range zero-filled on the way (fdgs_raster_params::acc_zero: the backward's accumulator)
};

// FORM (knob blend_fwd_form) = the inner loop.  0: one list entry per trip, staged as its three records.  1: the entries j and j + 1 per trip.
// What does not depend on the pixel's T -- both exponents, both alphas, 1 - alpha -- is evaluated for the two at once in packed f32 (one
// v_pk_* per operation and PAIR: the element-wise forms above, the roundings of form 0), speculatively for j + 1; then the part that depends
// on T runs for j and, unless the pixel stopped there, for j + 1, as form 0 does.  The three decisions (power > 0, alpha < 1/255,
// T (1 - alpha) < 1e-4) see the values form 0 computes, so every output bit is form 0's.  A round is staged as 128 pair records of five
// float4 -- (x x' y y') (cxx cxx' cxy cxy') (cyy cyy' opacity opacity') (r g b depth) (r' g' b' depth') -- so that the packed operands are the
// register pairs the reads deliver, read at five immediate offsets from one running address.  An odd list end: the entry behind it is
// staged as a copy of the last one (gid_of) and masked out of the sequential part.
template <int FORM>
__global__ void __launch_bounds__(256) render_fwd_kernel(RenderArgs a) {
    if (a.zfill)     // (the kernel is bound by its arithmetic: ~one 16-byte store per thread rides along for free, and a fill launch is gone)
        for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < a.zfill_n4; k += gridDim.x * 256u) a.zfill[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int tile = unit_lookup(a.order, a.per_xcd, blockIdx.x, a.gx, a.gy, 1, a.bh);
    if (tile < 0) return;
    __shared__ float4 sRec[FORM == 1 ? 640 : 768];
    float4 *const sA = sRec, *const sB = sRec + 256, *const sC = sRec + 512;      // (form 0)
    __shared__ uint32_t sTodo[4];
    const int t = threadIdx.x;
    const int x = (tile % a.gx) * TILE + (t & 15), y = (tile / a.gx) * TILE + (t >> 4);
    const bool inside = x < a.W && y < a.H;
    const float pxf = (float)x, pyf = (float)y;
    const uint2 range = a.ranges[tile];
    int toDo = (int)(range.y - range.x);
    const int rounds = (toDo + 255) / 256;
    bool done = !inside;
    float T = 1.0f, C0 = 0.f, C1 = 0.f, C2 = 0.f, Dp = 0.f;
    [[maybe_unused]] uint32_t contributor = 0;       // (form 0's count of the entries passed; form 1 derives it from the round and j)
    uint32_t last = 0;
    // staging pipeline (round 6; the backward has had it since round 3): list ids two rounds ahead, records one round ahead (the records'
    // addresses depend on the ids) -- the two dependent memory round trips of a round no longer sit between its barrier and its arithmetic
    const int n_list = (int)(range.y - range.x);
    auto gid_of = [&](int r) -> uint32_t {
        const int e = r * 256 + t;
        return a.pair_gid[range.x + (e < n_list ? e : n_list - 1)];
    };
    uint32_t g_cur = 0u, g_nxt = 0u;
    float4 rA, rB, rC;
    if (rounds > 0) {
        g_cur = gid_of(0);
        if (rounds > 1) g_nxt = gid_of(1);
        rA = a.recA[g_cur]; rB = a.recB[g_cur]; rC = a.recC[g_cur];
    }
    for (int r = 0; r < rounds; r++, toDo -= 256) {
        if (__syncthreads_count(done) == 256) break;
        if constexpr (FORM == 1) {               // entry t = half t & 1 of pair record t >> 1
            float* rec = reinterpret_cast<float*>(sRec + 5 * (t >> 1)) + (t & 1);
            rec[0] = rA.x; rec[2] = rA.y; rec[4] = rA.z; rec[6] = rA.w; rec[8] = rB.x; rec[10] = rB.y;
            sRec[5 * (t >> 1) + 3 + (t & 1)] = make_float4(rC.x, rC.y, rC.z, rB.z);
        } else {
            sA[t] = rA; sB[t] = rB; sC[t] = rC;  // (entries behind the end of the list are copies of its last entry: never read, j < lim)
        }
        __syncthreads();
        if (r + 1 < rounds) { g_cur = g_nxt; rA = a.recA[g_cur]; rB = a.recB[g_cur]; rC = a.recC[g_cur]; }
        if (r + 2 < rounds) g_nxt = gid_of(r + 2);
        const int lim = toDo < 256 ? toDo : 256;
        if constexpr (FORM == 1) {
            const uint32_t first = (uint32_t)r * 256u;       // entries in front of this round: form 0's `contributor` at entry j is first + j + 1
            const float4* q = sRec;
            for (int j = 0; !done && j < lim; j += 2, q += 5) {
                const float4 Q0 = q[0], Q1 = q[1], Q2 = q[2];
                float4 E0 = q[3];
                const float4 E1 = q[4];
                const v2f dx = v2f{Q0.x, Q0.y} - pxf, dy = v2f{Q0.z, Q0.w} - pyf;
                const v2f power = blend_power_e2(blend_power_xx_e2(v2f{Q1.x, Q1.y}, dx), blend_power_xy_e2(v2f{Q1.z, Q1.w}, dx), v2f{Q2.x, Q2.y}, dy);
                v2f alpha = v2f{Q2.z, Q2.w} * v2f{__expf(power[0]), __expf(power[1])};
                alpha[0] = fminf(FDGS_ALPHA_MAX, alpha[0]); alpha[1] = fminf(FDGS_ALPHA_MAX, alpha[1]);
                const v2f om = 1.0f - alpha;
                // (keeps the read of E0 with the four others at the top of the trip: sunk into the branch below it is a read of its own, with
                // its own address move and a full wait, in front of the first accumulation)
                asm volatile("" : "+v"(E0.x), "+v"(E0.y), "+v"(E0.z), "+v"(E0.w));
                if (!(power[0] > 0.0f) && !(alpha[0] < FDGS_ALPHA_MIN)) {
                    const float test_T = T * om[0];
                    if (test_T < FDGS_T_STOP) {
                        done = true;
                    } else {
                        const float w = alpha[0] * T;
                        C0 += E0.x * w; C1 += E0.y * w; C2 += E0.z * w; Dp += E0.w * w;
                        T = test_T;
                        last = first + (uint32_t)j + 1u;
                    }
                }
                if (!done && j + 1 < lim && !(power[1] > 0.0f) && !(alpha[1] < FDGS_ALPHA_MIN)) {
                    const float test_T = T * om[1];
                    if (test_T < FDGS_T_STOP) {
                        done = true;
                    } else {
                        const float w = alpha[1] * T;
                        C0 += E1.x * w; C1 += E1.y * w; C2 += E1.z * w; Dp += E1.w * w;
                        T = test_T;
                        last = first + (uint32_t)j + 2u;
                    }
                }
            }
        } else {
            for (int j = 0; !done && j < lim; j++) {
                contributor++;
                const float4 A = sA[j];
                const float4 B = sB[j];
                const float dx = A.x - pxf, dy = A.y - pyf;
                const float power = blend_power(blend_power_xx(A.z, dx), blend_power_xy(A.w, dx), B.x, dy);
                if (power > 0.0f) continue;
                const float alpha = fminf(FDGS_ALPHA_MAX, B.y * __expf(power));
                if (alpha < FDGS_ALPHA_MIN) continue;
                const float test_T = T * (1.0f - alpha);
                if (test_T < FDGS_T_STOP) { done = true; continue; }
                const float4 Cc = sC[j];
                const float w = alpha * T;
                C0 += Cc.x * w; C1 += Cc.y * w; C2 += Cc.z * w; Dp += B.z * w;
                T = test_T;
                last = contributor;
            }
        }
    }
    if (inside) {
        const size_t pix = (size_t)y * a.W + x, hw = (size_t)a.H * a.W;
        a.final_T[pix] = T; a.n_contrib[pix] = last;
        a.out_color[pix] = C0 + T * a.bg[0];
        a.out_color[hw + pix] = C1 + T * a.bg[1];
        a.out_color[2 * hw + pix] = C2 + T * a.bg[2];
        a.out_depth[pix] = Dp;
        if (a.out_alpha) a.out_alpha[pix] = 1.0f - T;        // (the T stored to final_T above: an empty list gives exactly 0)
    }
    {   // the tile's walk length for the backward (its work: the key of the backward's heaviest-first order)
        uint32_t m = inside ? last : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const uint32_t u = __shfl_xor(m, o, 64); m = u > m ? u : m; }
        __syncthreads();            // (the staging loop above may have been left at different points: sTodo is only touched here)
        if ((t & 63) == 0) sTodo[t >> 6] = m;
        __syncthreads();
        if (t == 0) {
            uint32_t q = sTodo[0]; q = sTodo[1] > q ? sTodo[1] : q; q = sTodo[2] > q ? sTodo[2] : q; q = sTodo[3] > q ? sTodo[3] : q;
            a.tile_todo[tile] = q;
        }
    }
}

#include "blend_replay.h"              // the replay walk: what the four kernels below share (ReplayArgs, replay_pixel ... replay_row)

// ---- the pick pass: which Gaussian a pixel shows, and the depth at which it turns opaque ----------------------------------------------
// A replay walk (blend_replay.h) that stages the ids beside recA and recB.  A += w is compiled without contraction: a product and a sum,
// the float32 running sum a blended colour channel of ones accumulates.  Per lane: T, A, the largest w and its id, the id and depth of the
// entry at which A reached alpha_cut.  No atomics, the four images are the only stores.  On an empty frame every pixel gets -1 / +0.
struct PickArgs : ReplayArgs {
    float alpha_cut;
    const int32_t* row_map;                  // opt [P]: the id written for Gaussian g
    int32_t* pick_id; float* pick_weight; int32_t* surface_id; float* surface_depth;      // each opt
};

__global__ void __launch_bounds__(256) render_pick_kernel(PickArgs a) {
#pragma clang fp contract(off)
    const ReplayPixel px = replay_pixel<true>(a);
    if (px.tile < 0) return;
    __shared__ float4 sA[256], sB[256];
    __shared__ uint32_t sG[256];
    const int t = threadIdx.x;
    const ReplayLengths len = replay_lengths<true>(a, px.tile, px.own);
    float T = 1.0f, A = 0.0f, best_w = 0.0f, s_depth = 0.0f;
    uint32_t best_g = 0xFFFFFFFFu, s_g = 0xFFFFFFFFu;
    int seen = 0;                            // entries of the list this lane has passed
    uint32_t g_cur = 0u, g_nxt = 0u;
    float4 rA, rB;
    if (len.rounds > 0) {
        g_cur = replay_gid(a, len, 0);
        if (len.rounds > 1) g_nxt = replay_gid(a, len, 1);
        rA = a.recA[g_cur]; rB = a.recB[g_cur];
    }
    for (int r = 0; r < len.rounds; r++) {
        if (__syncthreads_count(seen >= len.mine) == 256) break;
        sA[t] = rA; sB[t] = rB; sG[t] = g_cur;
        __syncthreads();
        if (r + 1 < len.rounds) { g_cur = g_nxt; rA = a.recA[g_cur]; rB = a.recB[g_cur]; }
        if (r + 2 < len.rounds) g_nxt = replay_gid(a, len, r + 2);
        const int rem = len.mine - seen;
        const int lim = rem < 256 ? rem : 256;
        for (int j = 0; j < lim; j++) {
            const float4 B = sB[j];
            replay_hit(sA[j], B, px.pxf, px.pyf, T, [&](float w, float T_behind) {
                A = A + w;
                if (w > best_w) { best_w = w; best_g = sG[j]; }              // (strictly: on a tie the entry in front stays)
                if (s_g == 0xFFFFFFFFu && A >= a.alpha_cut) { s_g = sG[j]; s_depth = B.z; }
                T = T_behind;
            });
        }
        seen += 256;
    }
    if (px.inside) {
        if (a.pick_id) a.pick_id[px.pix] = replay_row(a, best_g, a.row_map, 0xFFFFFFFFu);      // (no bound on the caller's ids)
        if (a.pick_weight) a.pick_weight[px.pix] = best_w;
        if (a.surface_id) a.surface_id[px.pix] = replay_row(a, s_g, a.row_map, 0xFFFFFFFFu);
        if (a.surface_depth) a.surface_depth[px.pix] = s_depth;
    }
}

// ---- the feature pass: C per-row channels blended in one walk ---------------------------------------------------------------------------
// A replay walk (blend_replay.h) with per-row VALUES in place of the colour record: channel c of a pixel is the sum over its contributors
// of values[row, c] * w, accumulated in list order as ONE explicit fused multiply-add per entry -- what the forward's `C0 += Cc.x * w`
// is compiled to (render_fwd_kernel is built with contraction) --, so a channel has the bits fdgs_render_fwd would blend for it over a zero
// background, and A = A + w is the pick pass's float32 running sum (the blend of a channel of ones: 1 * w is exact).
// Channels go in chunks of FEAT_CH = 16, blockIdx.y is the chunk and every chunk re-evaluates w: ONE launch for any C.  The thread that
// stages entry t also stages that entry's sixteen values (sV[4][256] float4 in LDS, loaded one round ahead with the records); a value whose
// channel is >= C or whose row is outside [0, rows) is staged as +0, and fma(+0, w, F) leaves F as it is.  In the inner loop every lane reads
// the same four float4 (broadcast reads).  The chunk size was measured (tools/features_timing.py): 8 keeps the pick pass's
// occupancy (54 VGPRs, 16.6 KB of LDS) and is faster up to C = 8 (config 4: 0.121 against 0.152 ms at C = 3), 16 (78 VGPRs, 24.8 KB: six
// waves per SIMD) pays the walk half as often and is faster from C = 9 on (0.161 against 0.215 ms at C = 16, 0.286 against 0.394 at C = 32).
// No atomics, the planes are the only stores.  On an empty frame every pixel gets +0.
#ifndef FDGS_FEAT_CH
#define FDGS_FEAT_CH 16                      // (8 at build time is the form it was measured against; a multiple of 4)
#endif
constexpr int FEAT_CH = FDGS_FEAT_CH, FEAT_V4 = FEAT_CH / 4;
static_assert(FEAT_CH % 4 == 0 && FEAT_CH >= 4, "whole float4 records");
struct FeatArgs : ReplayArgs {
    int C; const float* values; int value_stride; int rows;
    const int32_t* row_map;                  // opt [P]: the row of `values` Gaussian g takes
    float min_alpha;                         // < 0: raw sums; else F / A where A > min_alpha, 0 elsewhere
    float* features;                         // [C,H,W]
    float* alpha;                            // opt [H,W], written by chunk 0
};

__global__ void __launch_bounds__(256) render_features_kernel(FeatArgs a) {
#pragma clang fp contract(off)
    const ReplayPixel px = replay_pixel<true>(a);
    if (px.tile < 0) return;
    __shared__ float4 sA[256], sB[256], sV[FEAT_V4][256];
    const int t = threadIdx.x;
    const int c0 = (int)blockIdx.y * FEAT_CH;                                // this chunk's first channel
    const int nch = a.C - c0 < FEAT_CH ? a.C - c0 : FEAT_CH;                 // ... and how many of its sixteen exist (>= 1: the grid)
    const size_t hw = (size_t)a.H * a.W;
    const ReplayLengths len = replay_lengths<true>(a, px.tile, px.own);
    float T = 1.0f, A = 0.0f;
    float F[FEAT_CH];
#pragma unroll
    for (int k = 0; k < FEAT_CH; k++) F[k] = 0.0f;
    int seen = 0;                            // entries of the list this lane has passed
    // the values of Gaussian g in this chunk: 16-byte loads where the chunk is whole and its address allows them (values itself
    // is only 4-byte aligned: a row slice of a wider array), else one load per channel that exists
    auto values_of = [&](uint32_t g, float4 (&v)[FEAT_V4]) {
#pragma unroll
        for (int i = 0; i < FEAT_V4; i++) v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        const int32_t row = replay_row(a, g, a.row_map, (uint32_t)a.rows);
        if (row < 0) return;
        const float* src = a.values + (size_t)row * (size_t)a.value_stride + c0;
        if (nch == FEAT_CH && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
#pragma unroll
            for (int i = 0; i < FEAT_V4; i++) v[i] = reinterpret_cast<const float4*>(src)[i];
            return;
        }
        float q[FEAT_CH];
#pragma unroll
        for (int k = 0; k < FEAT_CH; k++) q[k] = k < nch ? src[k] : 0.0f;
#pragma unroll
        for (int i = 0; i < FEAT_V4; i++) v[i] = make_float4(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]);
    };
    uint32_t g_cur = 0u, g_nxt = 0u;
    float4 rA, rB, rV[FEAT_V4];
    if (len.rounds > 0) {
        g_cur = replay_gid(a, len, 0);
        if (len.rounds > 1) g_nxt = replay_gid(a, len, 1);
        rA = a.recA[g_cur]; rB = a.recB[g_cur]; values_of(g_cur, rV);
    }
    for (int r = 0; r < len.rounds; r++) {
        if (__syncthreads_count(seen >= len.mine) == 256) break;
        sA[t] = rA; sB[t] = rB;
#pragma unroll
        for (int i = 0; i < FEAT_V4; i++) sV[i][t] = rV[i];
        __syncthreads();
        if (r + 1 < len.rounds) { g_cur = g_nxt; rA = a.recA[g_cur]; rB = a.recB[g_cur]; values_of(g_cur, rV); }
        if (r + 2 < len.rounds) g_nxt = replay_gid(a, len, r + 2);
        const int rem = len.mine - seen;
        const int lim = rem < 256 ? rem : 256;
        for (int j = 0; j < lim; j++) {
            replay_hit(sA[j], sB[j], px.pxf, px.pyf, T, [&](float w, float T_behind) {
                A = A + w;
                T = T_behind;
#pragma unroll
                for (int i = 0; i < FEAT_V4; i++) {
                    const float4 V = sV[i][j];
                    F[4 * i] = __builtin_fmaf(V.x, w, F[4 * i]); F[4 * i + 1] = __builtin_fmaf(V.y, w, F[4 * i + 1]);
                    F[4 * i + 2] = __builtin_fmaf(V.z, w, F[4 * i + 2]); F[4 * i + 3] = __builtin_fmaf(V.w, w, F[4 * i + 3]);
                }
            });
        }
        seen += 256;
    }
    if (px.inside) {
        const bool normalize = a.min_alpha >= 0.0f;
        const bool ok = A > a.min_alpha;                                     // (a NaN A: false)
#pragma unroll
        for (int k = 0; k < FEAT_CH; k++) {
            const float q = F[k] / A;                                        // (IEEE division, as fdgs_motion_resolve's)
            if (k < nch) a.features[(size_t)(c0 + k) * hw + px.pix] = normalize ? (ok ? q : 0.0f) : F[k];
        }
        if (a.alpha && blockIdx.y == 0) a.alpha[px.pix] = A;
    }
}

#include "render_features_bwd.h"      // the feature pass's adjoint with respect to its values: render_features_bwd_kernel

// ---- wave64 all-reduce (sum): DPP inside rows, permlane swaps across rows; every lane ends with the total ----
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float wave_allsum(float v) {
    v += dpp_f<0xB1>(v);   // quad_perm [1,0,3,2]  : xor 1
    v += dpp_f<0x4E>(v);   // quad_perm [2,3,0,1]  : xor 2
    v += dpp_f<0x141>(v);  // row_half_mirror      : other quad of the 8
    v += dpp_f<0x140>(v);  // row_mirror           : other half of the 16
    {
        auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
    {
        auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
    return v;
}

// sum over the 16 lanes of a DPP row (= one 16-pixel line of the tile); every lane of the row ends with the row total
__device__ __forceinline__ float row_allsum(float v) {
    v += dpp_f<0xB1>(v);   // quad_perm [1,0,3,2]  : xor 1
    v += dpp_f<0x4E>(v);   // quad_perm [2,3,0,1]  : xor 2
    v += dpp_f<0x141>(v);  // row_half_mirror      : other quad of the 8
    v += dpp_f<0x140>(v);  // row_mirror           : other half of the 16
    return v;
}

// the largest of an unsigned word over the 64 lanes of a wave, wave_allsum's moves; every lane ends with it.  (The contribution pass takes
// the maximum of floats >= +0 on their BITS: fmaxf quiets its operands first, three instructions per step where v_max_u32 folds the DPP move.)
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
__device__ __forceinline__ uint32_t umax2(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t wave_allmax_u(uint32_t v) {
    v = umax2(v, dpp_u<0xB1>(v));
    v = umax2(v, dpp_u<0x4E>(v));
    v = umax2(v, dpp_u<0x141>(v));
    v = umax2(v, dpp_u<0x140>(v));
    {
        auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
        v = umax2(r[0], r[1]);
    }
    {
        auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
        v = umax2(r[0], r[1]);
    }
    return v;
}

// ---- the contribution pass: how much every Gaussian adds to the image ------------------------------------------------------------------
// A replay walk (blend_replay.h) that stages the ids, but what leaves the kernel is per GAUSSIAN, not per pixel: the sum and the maximum
// of v = w * pixel_weight over the pixels, the number of pixels with v > 0 and the number of tiles that hold one.  That is the blending
// backward's shape with three values per hit in place of nine: for a staged entry a wave in which no lane has v > 0 does nothing; otherwise
// it finishes sum, maximum and count over its 64 lanes in registers (DPP inside the rows, permlane swaps across them, a ballot's popcount)
// and lane 0 leaves them in the wave's own LDS slot sAcc[entry][wave] with ONE plain 16-byte store (no LDS atomics: ds_add_f32 sustains
// 0.33 lanes/clk/CU).  After the round the workgroup adds the four slots of every entry and issues at most ONE atomic per word of the
// Gaussian's 16-byte record and (tile, entry): four neighbouring lanes own the four words of one record -- f32 add, u32 max on the float's
// bits (v >= +0: the unsigned order of the bits is the order of the values), u32 add, u32 add of 1 -- so one wave's atomics of a pass cover
// 16 whole records.  (FDGS_CONTRIB_FLUSH_LANES = 1 at build time is the form it was measured against: one lane per record, four atomic
// instructions, each touching one word of 64 different records -- the same kernel time within 1 %, 0.212 against 0.213 ms on config 4:
// the flush is not where the time goes, the per-entry reductions are)  The walk loop runs to the WAVE's longest n_contrib so
// that every lane takes part in the reductions; a lane past its own end contributes v = 0.  Never launched on an empty frame.
#ifndef FDGS_CONTRIB_FLUSH_LANES
#define FDGS_CONTRIB_FLUSH_LANES 4
#endif
struct ContribArgs : ReplayArgs {
    const float* pixel_weight;               // opt [H*W]
    const int32_t* row_map;                  // opt [P]: the record Gaussian g is accumulated into
    uint32_t* rows;                          // [P] records of four words: weight_sum (f32), weight_max (f32), pixels, tiles
};

__global__ void __launch_bounds__(256) render_contrib_kernel(ContribArgs a) {
#pragma clang fp contract(off)
    const ReplayPixel px = replay_pixel<false>(a);
    if (px.tile < 0) return;
    __shared__ float4 sA[256], sB[256];
    __shared__ uint32_t sG[256];
    __shared__ uint4 sAcc[256 * 4];          // [entry][wave]: the bits of the sum, the bits of the maximum, the count, unused
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    uint32_t own = px.own;
    float m = 1.0f;
    if (a.pixel_weight) {
        m = px.inside ? a.pixel_weight[px.pix] : 0.0f;
        if (!(m > 0.0f)) own = 0u;           // zero, negative, NaN: no v of this pixel is > 0
    }
    const ReplayLengths len = replay_lengths<false>(a, px.tile, own);
    const int wave_mine = replay_wave_mine(len.mine);
    float T = 1.0f;
    int seen = 0;                            // entries of the list this lane has passed
    uint32_t g_cur = 0u, g_nxt = 0u;
    float4 rA, rB;
    if (len.rounds > 0) {
        g_cur = replay_gid(a, len, 0);
        if (len.rounds > 1) g_nxt = replay_gid(a, len, 1);
        rA = a.recA[g_cur]; rB = a.recB[g_cur];
    }
    for (int r = 0; r < len.rounds; r++) {
        if (__syncthreads_count(seen >= len.mine) == 256) break;
        const int left = len.todo - r * 256;
        const int staged = left < 256 ? left : 256;                         // entries of this round
        sA[t] = rA; sB[t] = rB; sG[t] = g_cur;
        for (int k = t; k < staged * 4; k += 256) sAcc[k] = make_uint4(0u, 0u, 0u, 0u);      // (an entry a wave does not hit keeps a zero slot)
        __syncthreads();
        if (r + 1 < len.rounds) { g_cur = g_nxt; rA = a.recA[g_cur]; rB = a.recB[g_cur]; }
        if (r + 2 < len.rounds) g_nxt = replay_gid(a, len, r + 2);
        const int rem = len.mine - seen;
        const int wave_rem = wave_mine - seen;
        const int lim = wave_rem < staged ? wave_rem : staged;
        for (int j = 0; j < lim; j++) {
            float v = 0.0f;
            if (j < rem) {
                const ReplayWeight e = replay_weight(sA[j], sB[j], px.pxf, px.pyf, T);
                v = e.w * m;                 // (skipped: +0 * m -- +0, or a NaN for an infinite m -- and not > 0 either way)
                T = e.T;
            }
            const bool hit = v > 0.0f;
            const unsigned long long hits = __ballot(hit);
            if (hits == 0ull) continue;                                      // (uniform over the wave)
            v = hit ? v : 0.0f;
            const float s = wave_allsum(v);
            const uint32_t mx = wave_allmax_u(__float_as_uint(v));           // (v >= +0: the order of the bits is the order of the values)
            if (lane == 0) sAcc[j * 4 + wv] = make_uint4(__float_as_uint(s), mx, (uint32_t)__popcll(hits), 0u);      // no other writer
        }
        seen += 256;
        __syncthreads();
        auto record_of = [&](int jj) -> uint32_t* {                          // where entry jj is accumulated, nullptr: dropped
            const int32_t row = replay_row(a, sG[jj], a.row_map, (uint32_t)a.P);
            return row >= 0 ? a.rows + (size_t)row * 4 : nullptr;
        };
#if FDGS_CONTRIB_FLUSH_LANES == 4
        const int sub = t & 3;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int jj = i * 64 + (t >> 2);
            if (jj >= staged) continue;
            const uint4 q0 = sAcc[jj * 4], q1 = sAcc[jj * 4 + 1], q2 = sAcc[jj * 4 + 2], q3 = sAcc[jj * 4 + 3];
            const uint32_t c = (q0.z + q1.z) + (q2.z + q3.z);
            if (c == 0u) continue;
            uint32_t* rec = record_of(jj);
            if (!rec) continue;
            if (sub == 0) {
                atomicAdd(reinterpret_cast<float*>(rec), (__uint_as_float(q0.x) + __uint_as_float(q1.x)) + (__uint_as_float(q2.x) + __uint_as_float(q3.x)));
            } else if (sub == 1) {
                atomicMax(rec + 1, umax2(umax2(q0.y, q1.y), umax2(q2.y, q3.y)));
            } else {
                atomicAdd(rec + sub, sub == 2 ? c : 1u);
            }
        }
#else
        if (t < staged) {
            const uint4 q0 = sAcc[t * 4], q1 = sAcc[t * 4 + 1], q2 = sAcc[t * 4 + 2], q3 = sAcc[t * 4 + 3];
            const uint32_t c = (q0.z + q1.z) + (q2.z + q3.z);
            uint32_t* rec = c ? record_of(t) : nullptr;
            if (rec) {
                atomicAdd(reinterpret_cast<float*>(rec), (__uint_as_float(q0.x) + __uint_as_float(q1.x)) + (__uint_as_float(q2.x) + __uint_as_float(q3.x)));
                atomicMax(rec + 1, umax2(umax2(q0.y, q1.y), umax2(q2.y, q3.y)));
                atomicAdd(rec + 2, c);
                atomicAdd(rec + 3, 1u);
            }
        }
#endif
    }
}

// Sums of ten values over the 64 lanes of a wave as a reduce-scatter.  xor-1 and xor-2 butterflies inside the quads halve the values
// per lane twice (lane bits 0,1 select which value a lane keeps); row_ror 4 / 8 add the four quads of a 16-lane row (they preserve
// lane & 3); v_permlane16_swap / v_permlane32_swap on PAIRS of values add the four rows while halving once more.  On return
//   lanes  0..15 hold sum(a[lane & 3]), lanes 16..31 sum(a[4 + (lane & 3)]), lanes 32..63 sum(a[8 + (lane & 1)]).
template <bool TEN>
__device__ __forceinline__ float wave_reduce_scatter10(float a0, float a1, float a2, float a3, float a4, float a5, float a6, float a7,
                                                       float a8, float a9, int lane) {
    const bool b0 = lane & 1, b1 = lane & 2;
    // (the DPP moves stay unconditional: a select between two DPP results is compiled into divergent branches)
    auto rs1 = [&](float lo, float hi) { const float keep = b0 ? hi : lo, send = b0 ? lo : hi; return keep + dpp_f<0xB1>(send); };   // lane ^ 1
    auto rs2 = [&](float lo, float hi) { const float keep = b1 ? hi : lo, send = b1 ? lo : hi; return keep + dpp_f<0x4E>(send); };   // lane ^ 2
    const float c0 = rs1(a0, a1), c1 = rs1(a2, a3), c2 = rs1(a4, a5), c3 = rs1(a6, a7);
    const float c4 = TEN ? rs1(a8, a9) : a8 + dpp_f<0xB1>(a8);
    float d0 = rs2(c0, c1), d1 = rs2(c2, c3), d2 = c4 + dpp_f<0x4E>(c4);
    d0 += dpp_f<0x124>(d0); d1 += dpp_f<0x124>(d1); d2 += dpp_f<0x124>(d2);     // row_ror:4
    d0 += dpp_f<0x128>(d0); d1 += dpp_f<0x128>(d1); d2 += dpp_f<0x128>(d2);     // row_ror:8
    // rows: swap16(x, y) leaves x' = [x.r0, y.r0, x.r2, y.r2], y' = [x.r1, y.r1, x.r3, y.r3]
    auto q01 = __builtin_amdgcn_permlane16_swap(__float_as_uint(d0), __float_as_uint(d1), false, false);
    const float e01 = __uint_as_float(q01[0]) + __uint_as_float(q01[1]);      // rows 0,2: d0 over a row pair; rows 1,3: d1
    auto q2 = __builtin_amdgcn_permlane16_swap(__float_as_uint(d2), __float_as_uint(d2), false, false);
    const float e2 = __uint_as_float(q2[0]) + __uint_as_float(q2[1]);
    // swap32(x, y) leaves x' = [x.lo, y.lo], y' = [x.hi, y.hi]
    auto q = __builtin_amdgcn_permlane32_swap(__float_as_uint(e01), __float_as_uint(e2), false, false);
    return __uint_as_float(q[0]) + __uint_as_float(q[1]);                      // lower half: e01 totals, upper half: e2 totals
}

// ... and of twelve (the blending backward with the absolute screen-space sums, values 10 and 11): the third group of four is whole, so it
// goes through both butterflies like the two others and the upper half-wave ends with sum(a[8 + (lane & 3)]).
__device__ __forceinline__ float wave_reduce_scatter12(float a0, float a1, float a2, float a3, float a4, float a5, float a6, float a7,
                                                       float a8, float a9, float a10, float a11, int lane) {
    const bool b0 = lane & 1, b1 = lane & 2;
    auto rs1 = [&](float lo, float hi) { const float keep = b0 ? hi : lo, send = b0 ? lo : hi; return keep + dpp_f<0xB1>(send); };   // lane ^ 1
    auto rs2 = [&](float lo, float hi) { const float keep = b1 ? hi : lo, send = b1 ? lo : hi; return keep + dpp_f<0x4E>(send); };   // lane ^ 2
    const float c0 = rs1(a0, a1), c1 = rs1(a2, a3), c2 = rs1(a4, a5), c3 = rs1(a6, a7), c4 = rs1(a8, a9), c5 = rs1(a10, a11);
    float d0 = rs2(c0, c1), d1 = rs2(c2, c3), d2 = rs2(c4, c5);
    d0 += dpp_f<0x124>(d0); d1 += dpp_f<0x124>(d1); d2 += dpp_f<0x124>(d2);     // row_ror:4
    d0 += dpp_f<0x128>(d0); d1 += dpp_f<0x128>(d1); d2 += dpp_f<0x128>(d2);     // row_ror:8
    auto q01 = __builtin_amdgcn_permlane16_swap(__float_as_uint(d0), __float_as_uint(d1), false, false);
    const float e01 = __uint_as_float(q01[0]) + __uint_as_float(q01[1]);
    auto q2 = __builtin_amdgcn_permlane16_swap(__float_as_uint(d2), __float_as_uint(d2), false, false);
    const float e2 = __uint_as_float(q2[0]) + __uint_as_float(q2[1]);
    auto q = __builtin_amdgcn_permlane32_swap(__float_as_uint(e01), __float_as_uint(e2), false, false);
    return __uint_as_float(q[0]) + __uint_as_float(q[1]);
}

struct RenderBwdArgs : BlendHead {
    const uint2* ranges; const uint32_t* pair_gid;
    const float4 *recA, *recB, *recC;
    const float* bg;
    const float* final_T; const uint32_t* n_contrib;
    const float *dL_dcolor, *dL_ddepth;
    const float* dL_dalpha;                  // opt [H*W]: gradient of the accumulated opacity A = 1 - final_T (fdgs_raster_bwd_alpha)
    float* gacc;  // [P,16] per-Gaussian gradient line: 0,1 mean2D (pixel units) | 2,3,4 conic xx,xy(half),yy | 5 opacity |
                  // 6,7,8 rgb | 9 depth | 10,11 sums over the pixels of |d L_pixel / d mean2D| (x, y; pixel units), written by the ABS
                  // instantiations only | 12..15 unused.  One 64-B line per Gaussian => one atomic line-op per (tile,Gaussian).
                  // All 16 floats of every line are zero when the kernel starts, whoever filled them: the forward's fill (RenderArgs::zfill,
                  // P * 4 float4) and the backward's own (raster_bwd_impl, P * 64 bytes) both cover the whole line, so slots 10..15 of a
                  // frame that does not ask stay zero and an ABS kernel adds into zeros.
};

// DEPTH: a gradient w.r.t. the depth image was handed in (dL_ddepth != NULL).  The reference's training loss never uses it
// (utils/scene_utils.py:29 reads depth under no_grad), so the common instantiation drops the depth accumulators, their
// row reduction and the tenth value of the per-Gaussian sums.
// ROUND = list entries staged per round (256 or 128).  The four waves of the tile meet in per-WAVE LDS slots
// sAcc[entry][wave][NV]: a wave that hits an entry finishes the sum over its 64 pixels in registers (DPP inside the 16-lane rows, then
// permlane16/32 swaps across the rows on the ONE value each lane carries) and lanes 0..NV-1 store it with a plain ds_write; the flush
// adds the four slots.  (Until round 3 the rows met in LDS float atomics on one shared slot -- ds_add_f32 sustains 0.33 lanes/clk/CU,
// profiles/r01_lds_atomic_microbench.txt, and rocprofv3 showed the waves waiting 39 % of their cycles.)
// ABS: the absolute screen-space sums as well (fdgs_raster_bwd_abs): |g_mx| and |g_my| of every pixel are values 10 and 11 of the same
// reductions, slots and flush (NV = 12 whatever DEPTH is, so that value k stays slot k of the line; the depth value is then a zero).
template <bool DEPTH, int ROUND, bool ABS = false>
__global__ void __launch_bounds__(256) render_bwd_kernel(RenderBwdArgs a) {
    const int tile = unit_lookup(a.order, a.per_xcd, blockIdx.x, a.gx, a.gy, 1, a.bh);
    if (tile < 0) return;
    constexpr int NV = ABS ? 12 : DEPTH ? 10 : 9;
    __shared__ float4 sA[ROUND], sB[ROUND], sC[ROUND];
    __shared__ uint32_t sGid[ROUND];
    __shared__ float sAcc[ROUND * 4 * NV];
    __shared__ uint32_t sMax[4];
    const int t = threadIdx.x, lane = t & 63;
    const int x = (tile % a.gx) * TILE + (t & 15), y = (tile / a.gx) * TILE + (t >> 4);
    const bool inside = x < a.W && y < a.H;
    const float pxf = (float)x, pyf = (float)y;
    const size_t pix = (size_t)y * a.W + x, hw = (size_t)a.H * a.W;
    const uint2 range = a.ranges[tile];
    const float T_final = inside ? a.final_T[pix] : 0.f;
    const uint32_t last_contributor = inside ? a.n_contrib[pix] : 0u;
    // the tile only ever needs the first max(n_contrib) entries of its list -- and each WAVE (a 16x4 pixel strip) only the first
    // max over its own 64 pixels: walking back to front, the entries behind that are skipped without being evaluated
    int wave_todo;
    {
        uint32_t m = last_contributor;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { uint32_t u = __shfl_xor(m, o, 64); m = u > m ? u : m; }
        if (lane == 0) sMax[t >> 6] = m;
        wave_todo = (int)m;
    }
    __syncthreads();
    uint32_t mx = sMax[0]; mx = sMax[1] > mx ? sMax[1] : mx; mx = sMax[2] > mx ? sMax[2] : mx; mx = sMax[3] > mx ? sMax[3] : mx;
    const int toDo = (int)mx;
    float dp0 = 0.f, dp1 = 0.f, dp2 = 0.f, ddep = 0.f;
    if (inside) {
        dp0 = a.dL_dcolor[pix]; dp1 = a.dL_dcolor[hw + pix]; dp2 = a.dL_dcolor[2 * hw + pix];
        if (DEPTH) ddep = a.dL_ddepth[pix];
    }
    // dA/dalpha_i = T_final / (1 - alpha_i) is the background term's factor with the sign turned: a gradient of the accumulated opacity
    // enters here, once per pixel, and the list walk below is the one a frame without it runs (x - 0 is x: the same bits when NULL)
    const float bgdot = (a.bg[0] * dp0 + a.bg[1] * dp1 + a.bg[2] * dp2) - ((inside && a.dL_dalpha) ? a.dL_dalpha[pix] : 0.f);
    float T = T_final, acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, accd = 0.f;
    float lc0 = 0.f, lc1 = 0.f, lc2 = 0.f, ld = 0.f, last_alpha = 0.f;
    const int rounds = (toDo + ROUND - 1) / ROUND;
    const int wv_ = t >> 6;
    for (int r = 0; r < rounds; r++) {
        const int e = toDo - 1 - (r * ROUND + t);  // list entry (0-based from the front) staged by this thread
        if (t < ROUND && e >= 0) {
            const uint32_t gid = a.pair_gid[range.x + e];
            sGid[t] = gid; sA[t] = a.recA[gid]; sB[t] = a.recB[gid]; sC[t] = a.recC[gid];
        }
        for (int k = t; k < ROUND * 4 * NV; k += 256) sAcc[k] = 0.f;      // (an entry a wave does not hit keeps a zero slot)
        __syncthreads();
        const int rem = toDo - r * ROUND;
        const int lim = rem < ROUND ? rem : ROUND;
        int j0 = toDo - wave_todo - r * ROUND;        // first staged entry of this round that one of the wave's pixels blended
        j0 = j0 < 0 ? 0 : j0;
        for (int j = j0; j < lim; j++) {
            const uint32_t ej = (uint32_t)(toDo - 1 - (r * ROUND + j));
            const float4 A = sA[j];
            const float4 B = sB[j];
            const float dx = A.x - pxf, dy = A.y - pyf;
            const float power = blend_power(blend_power_xx(A.z, dx), blend_power_xy(A.w, dx), B.x, dy);
            const float G = __expf(power);
            const float alpha = fminf(FDGS_ALPHA_MAX, B.y * G);
            const bool valid = (ej < last_contributor) && !(power > 0.0f) && !(alpha < FDGS_ALPHA_MIN);
            if (!__any(valid)) continue;
            float g_mx = 0.f, g_my = 0.f, g_cxx = 0.f, g_cxy = 0.f, g_cyy = 0.f, g_op = 0.f, g_c0 = 0.f, g_c1 = 0.f, g_c2 = 0.f,
                  g_d = 0.f;
            if (valid) {
                const float4 Cc = sC[j];
                // 1/(1-alpha) once (v_rcp_f32 + one Newton step, <= 1 ulp) for both divisions of the reference formula
                const float om = 1.0f - alpha;
                float inv = __builtin_amdgcn_rcpf(om);
                inv = fmaf(fmaf(-om, inv, 1.0f), inv, inv);
                T = T * inv;
                const float w = alpha * T;
                float dL_dalpha;
                acc0 = last_alpha * lc0 + (1.f - last_alpha) * acc0; lc0 = Cc.x;
                acc1 = last_alpha * lc1 + (1.f - last_alpha) * acc1; lc1 = Cc.y;
                acc2 = last_alpha * lc2 + (1.f - last_alpha) * acc2; lc2 = Cc.z;
                dL_dalpha = (Cc.x - acc0) * dp0 + (Cc.y - acc1) * dp1 + (Cc.z - acc2) * dp2;
                if (DEPTH) {
                    accd = last_alpha * ld + (1.f - last_alpha) * accd; ld = B.z;
                    dL_dalpha += (B.z - accd) * ddep;
                    g_d = w * ddep;
                }
                g_c0 = w * dp0; g_c1 = w * dp1; g_c2 = w * dp2;
                dL_dalpha *= T;
                last_alpha = alpha;
                dL_dalpha += (-T_final * inv) * bgdot;
                const float dL_dG = B.y * dL_dalpha;
                const float gdx = G * dx, gdy = G * dy;
                const float dG_ddelx = -gdx * A.z - gdy * A.w;
                const float dG_ddely = -gdy * B.x - gdx * A.w;
                g_mx = dL_dG * dG_ddelx; g_my = dL_dG * dG_ddely;
                g_cxx = -0.5f * gdx * dx * dL_dG; g_cxy = -0.5f * gdx * dy * dL_dG; g_cyy = -0.5f * gdy * dy * dL_dG;
                g_op = G * dL_dalpha;
            }
            // per-Gaussian sums over the wave's 64 pixels: DPP butterflies inside each 16-lane row (4 instructions per value); lane
            // `sub` of every row then picks value `sub` and the four rows are added with two permlane swaps on that ONE value
            [[maybe_unused]] float g_ax, g_ay;       // (ABS) this pixel's |g_mx|, |g_my| (an invalid pixel: |0|), summed like the others
            if constexpr (ABS) { g_ax = row_allsum(fabsf(g_mx)); g_ay = row_allsum(fabsf(g_my)); }
            g_mx = row_allsum(g_mx); g_my = row_allsum(g_my);
            g_cxx = row_allsum(g_cxx); g_cxy = row_allsum(g_cxy); g_cyy = row_allsum(g_cyy);
            g_op = row_allsum(g_op);
            g_c0 = row_allsum(g_c0); g_c1 = row_allsum(g_c1); g_c2 = row_allsum(g_c2);
            if (DEPTH) g_d = row_allsum(g_d);
            const int sub = lane & 15;
            float v = g_mx;
            v = sub == 1 ? g_my : v; v = sub == 2 ? g_cxx : v; v = sub == 3 ? g_cxy : v; v = sub == 4 ? g_cyy : v;
            v = sub == 5 ? g_op : v; v = sub == 6 ? g_c0 : v; v = sub == 7 ? g_c1 : v; v = sub == 8 ? g_c2 : v;
            if (DEPTH) v = sub == 9 ? g_d : v;
            if constexpr (ABS) { v = (!DEPTH && sub == 9) ? 0.f : v; v = sub == 10 ? g_ax : v; v = sub == 11 ? g_ay : v; }
            {
                auto q = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
                v = __uint_as_float(q[0]) + __uint_as_float(q[1]);
            }
            {
                auto q = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
                v = __uint_as_float(q[0]) + __uint_as_float(q[1]);
            }
            if (lane < NV) sAcc[(j * 4 + wv_) * NV + lane] = v;      // this wave's slot of entry j: plain store, no other writer
        }
        __syncthreads();
        // flush: 16 lanes own the 16-float gradient line of one staged Gaussian, so every atomic instruction covers four
        // whole 64-byte lines (measured: scattered float atomics cost ~1 line-op each at ~20 G line-ops/s on MI355X)
        {
            const int sub = lane & 15;
#pragma unroll 4
            for (int i = 0; i < ROUND / 16; i++) {
                const int jj = wv_ * (ROUND / 4) + i * 4 + (lane >> 4);
                if (jj < lim) {
                    float v = 0.f;
                    if (sub < NV) {
                        const float* sl = &sAcc[jj * 4 * NV + sub];
                        v = (sl[0] + sl[NV]) + (sl[2 * NV] + sl[3 * NV]);
                    }
                    if (v != 0.f) atomicAdd(&a.gacc[(size_t)sGid[jj] * 16 + sub], v);
                }
            }
        }
        __syncthreads();
    }
}

// ---- K7, strip form (round 3): ONE wave per workgroup, PPL pixels per lane ------------------------------------------------------
// The 256-thread form above is bound by VALU issue (a wave64 instruction holds its SIMD for four cycles): ~125 instructions per
// (wave, entry), of which ~50 are the cross-lane reduction of the nine per-Gaussian sums and ~15 the per-entry overhead -- paid once
// per 64 pixels.  Here a wave owns a 16 x (4*PPL) pixel strip of the tile, lane = (x, y0) with PPL pixels y0, y0+4, ... below each other:
//   * the lane's pixels share dx, so the per-Gaussian sums are first formed PER LANE as moments over dy (V0 = sum v, V1 = sum v*dy,
//     V2 = sum v*dy^2 with v = G * dL_dalpha) and turned into the six geometric sums once per lane, not once per pixel;
//   * the cross-lane reduction and the atomic line-op are paid once per 64*PPL pixels;
//   * the blending recurrences run branch-free (an invalid pixel blends alpha = 0, which leaves T and the running colour exactly
//     unchanged), in the un-lagged form acc' = alpha*c + (1-alpha)*acc (the same expression the lagged reference form evaluates one
//     entry later);
//   * a wave is its own workgroup: it stages its own 64 entries per round (records prefetched one round ahead, list ids two), never
//     waits for another wave, and sends its sums straight to the gradient line (lanes 0..NV-1, one atomic instruction per entry).
__device__ __forceinline__ v2f fma2(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ v2f splat2(float x) { return v2f{x, x}; }

// PPL = 2 * NP pixels per lane, held as NP float2 pairs so that the per-pixel arithmetic issues as v_pk_{mul,add,fma}_f32
// ABS: the absolute screen-space sums as well (fdgs_raster_bwd_abs).  The moments cannot give them -- the sign of a pixel's term depends on
// dy --, so a lane forms per pixel hx = cxx dx + cxy dy and hy = cyy dy + cxy dx (the pixel's d power / d mean, sign turned) on the pairs it
// holds and adds |v| |hx| and |v| |hy|; |opacity| is applied once per lane.  The two lane sums are values 10 and 11 of a twelve-value
// reduce-scatter and land in slots 10 and 11 of the line with the same atomic instruction.
template <bool DEPTH, int NP, bool ABS = false>
__global__ void __launch_bounds__(64) render_bwd_strip_kernel(RenderBwdArgs a) {
    constexpr int PPL = 2 * NP;
    constexpr int PARTS = 4 / PPL;
    const int unit = unit_lookup(a.order, a.per_xcd, blockIdx.x, a.gx, a.gy, PARTS, a.bh);
    if (unit < 0) return;
    const int tile = unit / PARTS, part = unit - tile * PARTS;
    __shared__ float4 sA[64], sB[64], sC[64];
    __shared__ uint32_t sGid[64];
    const int lane = threadIdx.x;
    const int x = (tile % a.gx) * TILE + (lane & 15);
    const int y0 = (tile / a.gx) * TILE + part * (4 * PPL) + (lane >> 4);
    const float pxf = (float)x;
    const size_t hw = (size_t)a.H * a.W;
    // which of the per-Gaussian sums this lane holds after wave_reduce_scatter10, and whether it is the lane that sends it
    // (ABS, wave_reduce_scatter12: the upper half-wave holds 8 + (lane & 3); lanes 34 and 35 send the absolute sums, lane 33 the depth's)
    const int slot = lane < 16 ? (lane & 3) : lane < 32 ? 4 + (lane & 3) : 8 + (lane & (ABS ? 3 : 1));
    const bool slot_on = (lane & 15) < 4 && (lane < 32 || (lane < 48 && ((lane & 15) < (DEPTH ? 2 : 1) || (ABS && (lane & 15) >= 2))));
    const uint2 range = a.ranges[tile];
    v2f py[NP], T[NP], tfb[NP], dp0[NP], dp1[NP], dp2[NP], ddep[NP], acc0[NP], acc1[NP], acc2[NP], accd[NP];
    v2f dal[NP];                         // dL/dA of the pixels (0 without a.dL_dalpha): only lives until tfb is formed
    uint32_t lastc[PPL];
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < PPL; i++) {
        const int y = y0 + 4 * i;
        const bool inside = x < a.W && y < a.H;
        const size_t pix = (size_t)y * a.W + x;
        const int p = i >> 1, c = i & 1;
        py[p][c] = (float)y;
        T[p][c] = inside ? a.final_T[pix] : 0.f;
        lastc[i] = inside ? a.n_contrib[pix] : 0u;
        dp0[p][c] = inside ? a.dL_dcolor[pix] : 0.f;
        dp1[p][c] = inside ? a.dL_dcolor[hw + pix] : 0.f;
        dp2[p][c] = inside ? a.dL_dcolor[2 * hw + pix] : 0.f;
        ddep[p][c] = (DEPTH && inside) ? a.dL_ddepth[pix] : 0.f;
        dal[p][c] = (inside && a.dL_dalpha) ? a.dL_dalpha[pix] : 0.f;
        m = lastc[i] > m ? lastc[i] : m;
    }
#pragma unroll
    for (int p = 0; p < NP; p++) {
        // (dA/dalpha_i = T_final / (1 - alpha_i), the background term's factor with the sign turned: x - 0 is x, the same bits without it)
        tfb[p] = -T[p] * ((a.bg[0] * dp0[p] + a.bg[1] * dp1[p] + a.bg[2] * dp2[p]) - dal[p]);
        acc0[p] = acc1[p] = acc2[p] = accd[p] = splat2(0.f);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t u = __shfl_xor(m, o, 64); m = u > m ? u : m; }
    const int todo = (int)m;             // the strip only ever needs the first max(n_contrib) entries of the tile's list
    if (todo == 0) return;
    const int rounds = (todo + 63) >> 6;
    // staging pipeline: list ids two rounds ahead, records one round ahead (the records' addresses depend on the ids)
    auto gid_of = [&](int r) -> uint32_t {
        const int e = todo - 1 - (r * 64 + lane);
        return a.pair_gid[range.x + (e >= 0 ? e : 0)];
    };
    // (staging the records with global_load_lds_dwordx4 into a second LDS buffer frees their 12 registers -- 90 VGPRs, five waves per
    // SIMD -- and measured SLOWER, 0.341 vs 0.313 ms: the round-start vmcnt(0) also waits for the round's 64 atomics, and with a
    // counted wait hipcc still puts a vmcnt(0) in front of every LDS read that may alias an outstanding DMA -- one per list entry;
    // profiles/r03j_bench_cfg4_rbwd_glds.json)
    uint32_t g_cur = gid_of(0), g_nxt = rounds > 1 ? gid_of(1) : 0u;
    float4 rA = a.recA[g_cur], rB = a.recB[g_cur], rC = a.recC[g_cur];
    for (int r = 0; r < rounds; r++) {
        __syncthreads();                 // (one wave: orders the previous round's LDS reads before these writes)
        sGid[lane] = g_cur; sA[lane] = rA; sB[lane] = rB; sC[lane] = rC;
        __syncthreads();
        if (r + 1 < rounds) { g_cur = g_nxt; rA = a.recA[g_cur]; rB = a.recB[g_cur]; rC = a.recC[g_cur]; }
        if (r + 2 < rounds) g_nxt = gid_of(r + 2);
        const int rem = todo - r * 64;
        const int lim = rem < 64 ? rem : 64;
        for (int j = 0; j < lim; j++) {
            const uint32_t ej = (uint32_t)(todo - 1 - (r * 64 + j));
            const float4 A = sA[j];
            const float4 B = sB[j];
            const float dx = A.x - pxf;
            v2f dy[NP], G[NP], alpha[NP];
            bool valid[PPL], any = false;
            {
                const float u1 = blend_power_xx(A.z, dx);
                const float cx = blend_power_xy(A.w, dx);
#pragma unroll
                for (int p = 0; p < NP; p++) {
                    dy[p] = splat2(A.y) - py[p];
                    const v2f power = blend_power2(u1, cx, B.x, dy[p]);
                    G[p][0] = __expf(fminf(power[0], 0.0f));      // (power > 0 is invalid below; the clamp only keeps G finite)
                    G[p][1] = __expf(fminf(power[1], 0.0f));
                    alpha[p] = B.y * G[p];
                    alpha[p][0] = fminf(FDGS_ALPHA_MAX, alpha[p][0]);
                    alpha[p][1] = fminf(FDGS_ALPHA_MAX, alpha[p][1]);
#pragma unroll
                    for (int c = 0; c < 2; c++) {
                        valid[2 * p + c] = (ej < lastc[2 * p + c]) && !(power[c] > 0.0f) && !(alpha[p][c] < FDGS_ALPHA_MIN);
                        any = any || valid[2 * p + c];
                    }
                }
            }
            if (!__any(any)) continue;
            const float4 Cc = sC[j];
            v2f V0 = splat2(0.f), V1 = V0, V2 = V0, gc0 = V0, gc1 = V0, gc2 = V0, gd = V0;
            [[maybe_unused]] v2f Ax = V0, Ay = V0;       // (ABS) sums of |v| |hx|, |v| |hy| over the lane's pixels
            [[maybe_unused]] const float cxdx = A.z * dx, cydx = A.w * dx;
#pragma unroll
            for (int p = 0; p < NP; p++) {
                v2f al;
                al[0] = valid[2 * p] ? alpha[p][0] : 0.f;
                al[1] = valid[2 * p + 1] ? alpha[p][1] : 0.f;
                // 1/(1-alpha) once (v_rcp_f32 + one Newton step, <= 1 ulp) for both divisions of the reference formula
                const v2f om = splat2(1.0f) - al;
                v2f inv;
                inv[0] = __builtin_amdgcn_rcpf(om[0]); inv[1] = __builtin_amdgcn_rcpf(om[1]);
                inv = fma2(fma2(-om, inv, splat2(1.0f)), inv, inv);
                T[p] = T[p] * inv;
                const v2f w = al * T[p];
                v2f dLda = fma2(splat2(Cc.z) - acc2[p], dp2[p], fma2(splat2(Cc.y) - acc1[p], dp1[p], (splat2(Cc.x) - acc0[p]) * dp0[p]));
                if (DEPTH) {
                    dLda = fma2(splat2(B.z) - accd[p], ddep[p], dLda);
                    accd[p] = fma2(al, splat2(B.z), om * accd[p]);
                    gd = fma2(w, ddep[p], gd);
                }
                acc0[p] = fma2(al, splat2(Cc.x), om * acc0[p]);
                acc1[p] = fma2(al, splat2(Cc.y), om * acc1[p]);
                acc2[p] = fma2(al, splat2(Cc.z), om * acc2[p]);
                gc0 = fma2(w, dp0[p], gc0); gc1 = fma2(w, dp1[p], gc1); gc2 = fma2(w, dp2[p], gc2);
                dLda = fma2(dLda, T[p], tfb[p] * inv);
                v2f v = G[p] * dLda;
                v[0] = valid[2 * p] ? v[0] : 0.f;
                v[1] = valid[2 * p + 1] ? v[1] : 0.f;
                const v2f vy = v * dy[p];
                V0 += v; V1 += vy; V2 = fma2(vy, dy[p], V2);
                if constexpr (ABS) {
                    const v2f hx = fma2(splat2(A.w), dy[p], splat2(cxdx)), hy = fma2(splat2(B.x), dy[p], splat2(cydx));
                    const v2f av = __builtin_elementwise_abs(v);
                    Ax = fma2(av, __builtin_elementwise_abs(hx), Ax); Ay = fma2(av, __builtin_elementwise_abs(hy), Ay);
                }
            }
            // the lane's six geometric sums from its moments over dy (dL_dG * G = opacity * v)
            const float u0 = B.y * (V0[0] + V0[1]), u1 = B.y * (V1[0] + V1[1]), u2 = B.y * (V2[0] + V2[1]);
            const float ux = u0 * dx;
            float g_mx = -(A.z * ux + A.w * u1), g_my = -(B.x * u1 + A.w * ux);
            float g_cxx = -0.5f * ux * dx, g_cxy = -0.5f * u1 * dx, g_cyy = -0.5f * u2;
            float g_op = V0[0] + V0[1];
            float g_c0 = gc0[0] + gc0[1], g_c1 = gc1[0] + gc1[1], g_c2 = gc2[0] + gc2[1], g_d = gd[0] + gd[1];
            // nine (ten) sums over the wave's 64 lanes as a reduce-scatter: each butterfly step halves the number of values a lane
            // carries (36 instructions instead of 50 for nine all-reduces + select); lane `slot_lane` ends with value `slot`
            float v;
            if constexpr (ABS) {
                const float aop = fabsf(B.y);
                v = wave_reduce_scatter12(g_mx, g_my, g_cxx, g_cxy, g_cyy, g_op, g_c0, g_c1, g_c2, g_d, aop * (Ax[0] + Ax[1]), aop * (Ay[0] + Ay[1]), lane);
            } else {
                v = wave_reduce_scatter10<DEPTH>(g_mx, g_my, g_cxx, g_cxy, g_cyy, g_op, g_c0, g_c1, g_c2, g_d, lane);
            }
            if (slot_on && v != 0.f) atomicAdd(&a.gacc[(size_t)sGid[j] * 16 + slot], v);
        }
    }
}

// do the blending kernels of this image take their tiles heaviest-first (the knob is on and an XCD's tiles fit its LDS sort)?
static bool tiles_ordered(const ImgLayout& il) { return g_tune.tile_order && il.per_xcd <= TILE_ORDER_MAX && il.per_xcd >= 1; }

// launches tile_order_kernel where tiles_ordered; returns the order to hand to the kernel (or nullptr)
static const uint32_t* make_tile_order(hipStream_t stream, int mode, const ImgLayout& il, const void* img, void* img_w) {
    if (!tiles_ordered(il)) return nullptr;
    uint32_t* order = at<uint32_t>(img_w, mode == 0 ? il.order_f : il.order_b);
    FDGS_TIMED("tile_order", stream);
    hipLaunchKernelGGL(tile_order_kernel, dim3(8), dim3(1024), 0, stream, mode, il.gx, il.gy, XCD_ROWS, il.per_xcd, at<uint2>(img, il.ranges),
                       at<uint32_t>(img, il.todo), order);
    return order;
}

int launch_tile_scan_order(hipStream_t stream, const ImgLayout& il, const uint32_t* counts, void* img, uint32_t cap, int debug, bool* order_made) {
    const bool ordered = tiles_ordered(il);
    {
        FDGS_TIMED("tile_scan", stream);
        hipLaunchKernelGGL(tile_scan_order_kernel, dim3(ordered ? 9 : 1), dim3(1024), 0, stream, counts, (uint32_t)(il.gx * il.gy), at<uint2>(img, il.ranges), cap,
                           il.gx, il.gy, XCD_ROWS, il.per_xcd, at<uint32_t>(img, il.order_f));
    }
    FDGS_LAUNCH_CHECK("tile_scan", debug, stream);
    if (order_made) *order_made = ordered;
    return FDGS_OK;
}

// what both blending launchers set from the frame's buffers (Args = RenderArgs with a writable img, RenderBwdArgs with a const one; the
// replay passes have fill_replay_args); `order` stays with the launcher: making it is a launch
template <typename Args, typename Img>
static ImgLayout fill_blend_args(Args& a, const fdgs_raster_params* p, const void* geom, const void* binning, Img* img, uint32_t R) {
    const GeomLayout gl = geom_layout(p->P);
    const BinLayout bl = bin_layout(R);
    const ImgLayout il = img_layout(p->W, p->H);
    a.W = p->W; a.H = p->H; a.gx = il.gx; a.gy = il.gy; a.bh = XCD_ROWS; a.per_xcd = il.per_xcd;
    a.ranges = at<uint2>(img, il.ranges); a.pair_gid = binning ? at<uint32_t>(binning, bl.gid0) : nullptr;
    a.recA = at<float4>(geom, gl.recA); a.recB = at<float4>(geom, gl.recB); a.recC = at<float4>(geom, gl.recC);
    a.bg = p->bg; a.final_T = at<float>(img, il.final_T); a.n_contrib = at<uint32_t>(img, il.n_contrib);
    return il;
}

// what the four replay entry points (fdgs_render_pick / _features / _features_bwd / _contrib) check first; `pointers`: the call's own
// required pointers, p among them, are all there
static int check_replay_call(bool pointers, const char* null_msg, const fdgs_raster_params* p) {
    FDGS_REQUIRE(pointers, null_msg);
    FDGS_REQUIRE(p->P >= 0 && p->W >= 1 && p->H >= 1, "bad P/W/H");
    FDGS_REQUIRE((p->W + TILE - 1) / TILE < 65536 && (p->H + TILE - 1) / TILE < 65536, "image too large");
    return FDGS_OK;
}

// every field of a replay kernel's ReplayArgs from the finished frame's buffers.  `order` is the forward's own heaviest-first order where
// fdgs_render_fwd wrote one (make_tile_order's condition), never rebuilt here.  Of *p only P, W and H are read and none of its pointers is
// looked at: a later frame may have overwritten what they named.
static void fill_replay_args(ReplayArgs& a, const fdgs_raster_params* p, const void* geom, const void* binning, const void* img, uint32_t R) {
    const GeomLayout gl = geom_layout(p->P);
    const BinLayout bl = bin_layout(R);
    const ImgLayout il = img_layout(p->W, p->H);
    a.W = p->W; a.H = p->H; a.gx = il.gx; a.gy = il.gy; a.bh = XCD_ROWS; a.per_xcd = il.per_xcd;
    a.empty = (p->P == 0 || R == 0) ? 1 : 0;
    a.order = !a.empty && tiles_ordered(il) ? at<uint32_t>(img, il.order_f) : nullptr;
    a.tile_todo = at<uint32_t>(img, il.todo); a.ranges = at<uint2>(img, il.ranges); a.pair_gid = at<uint32_t>(binning, bl.gid0);
    a.recA = at<float4>(geom, gl.recA); a.recB = at<float4>(geom, gl.recB);
    a.n_contrib = at<uint32_t>(img, il.n_contrib);
    a.R = R; a.P = p->P;
}

// The blending backward's form.  ppl = pixels per lane of the strip form (one wave per workgroup, 4 / ppl of them per tile); anything but
// 2 or 4 = the 256-thread form (128 entries staged per round keeps six workgroups per CU at 25 KB of LDS each).  depth: dL_ddepth was
// handed in.  abs: the absolute screen-space sums too (slots 10, 11); a frame without them launches the instantiations it always launched.
// (The tables name the instantiations in the order the device code has always listed them.)
static void launch_render_bwd(hipStream_t stream, int ppl, bool depth, bool abs, const RenderBwdArgs& a) {
    using Kernel = void (*)(RenderBwdArgs);
    static const Kernel strip[2][2] = {{render_bwd_strip_kernel<true, 1>, render_bwd_strip_kernel<true, 2>},
                                       {render_bwd_strip_kernel<false, 1>, render_bwd_strip_kernel<false, 2>}};
    static const Kernel whole[2] = {render_bwd_kernel<true, 128>, render_bwd_kernel<false, 128>};
    static const Kernel strip_abs[2][2] = {{render_bwd_strip_kernel<true, 1, true>, render_bwd_strip_kernel<true, 2, true>},
                                           {render_bwd_strip_kernel<false, 1, true>, render_bwd_strip_kernel<false, 2, true>}};
    static const Kernel whole_abs[2] = {render_bwd_kernel<true, 128, true>, render_bwd_kernel<false, 128, true>};
    if (ppl == 2 || ppl == 4)
        hipLaunchKernelGGL((abs ? strip_abs : strip)[depth ? 0 : 1][ppl / 4], dim3(unit_grid(a.gx, a.gy, 4 / ppl, a.bh)), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL((abs ? whole_abs : whole)[depth ? 0 : 1], dim3(unit_grid(a.gx, a.gy, 1, a.bh)), dim3(256), 0, stream, a);
}

}  // namespace fdgs

using namespace fdgs;

namespace fdgs {
int render_fwd_impl(void* stream_, const fdgs_raster_params* p, const void* geom, const void* binning, void* img, uint32_t R, float* out_color,
                    float* out_depth, bool order_made, float* out_alpha) {
    int rc = validate_raster_params(p);
    if (rc) return rc;
    FDGS_REQUIRE(geom && img && out_color && out_depth && (binning || R == 0), "NULL buffer");
    FDGS_REQUIRE(aligned_to(out_alpha, 4), "out_alpha must be 4-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    RenderArgs a{};
    const ImgLayout il = fill_blend_args(a, p, geom, binning, img, R);
    a.out_color = out_color; a.out_depth = out_depth; a.out_alpha = out_alpha;
    a.tile_todo = at<uint32_t>(img, il.todo);
    a.zfill = reinterpret_cast<float4*>(p->acc_zero); a.zfill_n4 = (uint32_t)p->P * 4u;
    a.order = R == 0 ? nullptr : order_made ? at<uint32_t>(img, il.order_f) : make_tile_order(stream, 0, il, img, img);
    {
        FDGS_TIMED("render_fwd", stream);
        hipLaunchKernelGGL(g_tune.blend_fwd_form == 1 ? render_fwd_kernel<1> : render_fwd_kernel<0>, dim3(unit_grid(a.gx, a.gy, 1, a.bh)), dim3(256), 0, stream, a);
    }
    FDGS_LAUNCH_CHECK("render_fwd", p->debug, stream);
    return FDGS_OK;
}
}  // namespace fdgs

extern "C" int fdgs_render_fwd(void* stream_, const fdgs_raster_params* p, const void* geom, const void* binning, void* img,
                               uint32_t R, float* out_color, float* out_depth) {
    return render_fwd_impl(stream_, p, geom, binning, img, R, out_color, out_depth, false, nullptr);
}

extern "C" int fdgs_render_fwd_alpha(void* stream_, const fdgs_raster_params* p, const void* geom, const void* binning, void* img,
                                     uint32_t R, float* out_color, float* out_depth, float* out_alpha) {
    return render_fwd_impl(stream_, p, geom, binning, img, R, out_color, out_depth, false, out_alpha);
}

extern "C" int fdgs_render_pick(void* stream_, const fdgs_raster_params* p, const void* geom, const void* binning, const void* img,
                                uint32_t R, float alpha_cut, const int32_t* row_map_opt, const fdgs_pick_out* out) {
    if (int rc = check_replay_call(p && geom && binning && img && out, "NULL pointer (params, geom, binning, img and out)", p)) return rc;
    FDGS_REQUIRE(alpha_cut > 0.0f && alpha_cut <= 1.0f, "bad alpha_cut (in (0, 1]; a NaN is refused)");
    FDGS_REQUIRE(out->pick_id || out->pick_weight || out->surface_id || out->surface_depth, "NULL pointer (at least one output)");
    FDGS_REQUIRE(aligned_to(out->pick_id, 4) && aligned_to(out->pick_weight, 4) && aligned_to(out->surface_id, 4) &&
                     aligned_to(out->surface_depth, 4) && aligned_to(row_map_opt, 4), "arrays must be 4-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    PickArgs a{};
    fill_replay_args(a, p, geom, binning, img, R);
    a.alpha_cut = alpha_cut; a.row_map = row_map_opt;
    a.pick_id = out->pick_id; a.pick_weight = out->pick_weight; a.surface_id = out->surface_id; a.surface_depth = out->surface_depth;
    {
        FDGS_TIMED("render_pick", stream);
        hipLaunchKernelGGL(render_pick_kernel, dim3(unit_grid(a.gx, a.gy, 1, a.bh)), dim3(256), 0, stream, a);
    }
    FDGS_LAUNCH_CHECK("render_pick", p->debug, stream);
    return FDGS_OK;
}

extern "C" int fdgs_render_features(void* stream_, const fdgs_raster_params* p, const void* geom, const void* binning, const void* img,
                                    uint32_t R, int C, const float* values, int value_stride, int rows, const int32_t* row_map_opt,
                                    float min_alpha, float* features, float* alpha_opt) {
    if (int rc = check_replay_call(p && geom && binning && img && values && features, "NULL pointer (params, geom, binning, img, values and features)", p))
        return rc;
    FDGS_REQUIRE(C >= 1 && C <= 8 * 65535, "bad C (1 .. 8 * 65535 channels)");
    FDGS_REQUIRE(value_stride >= C, "bad value_stride (at least C floats per row)");
    FDGS_REQUIRE(rows >= 0, "bad rows (negative)");
    FDGS_REQUIRE(aligned_to(values, 4) && aligned_to(row_map_opt, 4) && aligned_to(features, 4) && aligned_to(alpha_opt, 4),
                 "arrays must be 4-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    FeatArgs a{};
    fill_replay_args(a, p, geom, binning, img, R);
    a.C = C; a.values = values; a.value_stride = value_stride; a.rows = rows; a.row_map = row_map_opt;
    a.min_alpha = min_alpha >= 0.0f ? min_alpha : -1.0f;                    // (negative or NaN: raw sums)
    a.features = features; a.alpha = alpha_opt;
    {
        FDGS_TIMED("render_features", stream);
        hipLaunchKernelGGL(render_features_kernel, dim3(unit_grid(a.gx, a.gy, 1, a.bh), (C + FEAT_CH - 1) / FEAT_CH), dim3(256), 0, stream, a);
    }
    FDGS_LAUNCH_CHECK("render_features", p->debug, stream);
    return FDGS_OK;
}

extern "C" int fdgs_render_features_bwd(void* stream_, const fdgs_raster_params* p, const void* geom, const void* binning, const void* img,
                                        uint32_t R, int C, const float* dL_dfeatures, const float* alpha_opt, float min_alpha,
                                        const int32_t* row_map_opt, int rows, float* dvalues, int dvalue_stride) {
    if (int rc = check_replay_call(p && geom && binning && img && dL_dfeatures && dvalues,
                                   "NULL pointer (params, geom, binning, img, dL_dfeatures and dvalues)", p))
        return rc;
    FDGS_REQUIRE(C >= 1 && C <= 8 * 65535, "bad C (1 .. 8 * 65535 channels)");
    FDGS_REQUIRE(dvalue_stride >= C, "bad dvalue_stride (at least C floats per row)");
    FDGS_REQUIRE(rows >= 0, "bad rows (negative)");
    const bool normalized = min_alpha >= 0.0f;                              // (negative or NaN: the forward wrote raw sums)
    FDGS_REQUIRE(!normalized || alpha_opt, "NULL alpha_opt with min_alpha >= 0 (the alpha image the normalised forward wrote)");
    FDGS_REQUIRE(aligned_to(dL_dfeatures, 4) && aligned_to(alpha_opt, 4) && aligned_to(row_map_opt, 4) && aligned_to(dvalues, 4),
                 "arrays must be 4-byte aligned");
    if (p->P == 0 || R == 0) return FDGS_OK;          // nothing was blended: nothing is accumulated, nothing is launched
    hipStream_t stream = (hipStream_t)stream_;
    // (of *p only P, W, H and debug are read and none of its pointers is looked at: a later frame may have overwritten what they named)
    FeatBwdArgs a{};
    fill_replay_args(a, p, geom, binning, img, R);
    a.C = C; a.grad = dL_dfeatures; a.alpha = normalized ? alpha_opt : nullptr; a.min_alpha = normalized ? min_alpha : -1.0f;
    a.row_map = row_map_opt; a.rows = rows; a.dvalues = dvalues; a.dvalue_stride = dvalue_stride;
    {
        FDGS_TIMED("render_features_bwd", stream);
        hipLaunchKernelGGL(render_features_bwd_kernel, dim3(unit_grid(a.gx, a.gy, 1, a.bh), (C + FEAT_CH - 1) / FEAT_CH), dim3(256), 0, stream, a);
    }
    FDGS_LAUNCH_CHECK("render_features_bwd", p->debug, stream);
    return FDGS_OK;
}

extern "C" int fdgs_render_contrib(void* stream_, const fdgs_raster_params* p, const void* geom, const void* binning, const void* img,
                                   uint32_t R, const float* pixel_weight_opt, const int32_t* row_map_opt, fdgs_contrib_row* rows) {
    if (int rc = check_replay_call(p && geom && binning && img && rows, "NULL pointer (params, geom, binning, img and rows)", p)) return rc;
    FDGS_REQUIRE(aligned_to(rows, 16), "rows must be 16-byte aligned");
    FDGS_REQUIRE(aligned_to(pixel_weight_opt, 4) && aligned_to(row_map_opt, 4), "pixel_weight_opt and row_map_opt must be 4-byte aligned");
    if (p->P == 0 || R == 0) return FDGS_OK;          // nothing was blended: nothing is accumulated, nothing is launched
    hipStream_t stream = (hipStream_t)stream_;
    ContribArgs a{};
    fill_replay_args(a, p, geom, binning, img, R);
    a.pixel_weight = pixel_weight_opt; a.row_map = row_map_opt;
    a.rows = reinterpret_cast<uint32_t*>(rows);
    {
        FDGS_TIMED("render_contrib", stream);
        hipLaunchKernelGGL(render_contrib_kernel, dim3(unit_grid(a.gx, a.gy, 1, a.bh)), dim3(256), 0, stream, a);
    }
    FDGS_LAUNCH_CHECK("render_contrib", p->debug, stream);
    return FDGS_OK;
}

// fdgs_raster_bwd (dL_dalpha == nullptr), fdgs_raster_bwd_alpha and fdgs_raster_bwd_aa (antialiasing: the blending backward is the same --
// its opacity sum is then the gradient of the compensated opacity -- and the per-Gaussian chain rule carries the compensation's)
// ... and fdgs_raster_bwd_abs (means2D_abs [P,3], opt: the blending backward also sums the absolute screen-space terms, slots 10 and 11 of
// the line, and the chain rule writes them out; a row no pixel blended reads the zeros the line was filled with)
static int raster_bwd_impl(void* stream_, const fdgs_raster_params* p, const void* geom, const void* binning, const void* img, uint32_t R,
                           const fdgs_raster_grads* g, const float* dL_dalpha, bool antialiasing = false, float* means2D_abs = nullptr) {
    int rc = validate_raster_params(p);
    if (rc) return rc;
    FDGS_REQUIRE(g && geom && img && (binning || R == 0), "NULL buffer");
    FDGS_REQUIRE(aligned_to(dL_dalpha, 4), "dL_dalpha must be 4-byte aligned");
    FDGS_REQUIRE(aligned_to(means2D_abs, 4), "dL_dmeans2D_abs must be 4-byte aligned");
    if (p->P == 0) return FDGS_OK;      // an empty set: no row to write (its optional per-row inputs may come without their gradient buffers)
    if (g->deform_epilogue) {     // the per-Gaussian results go to the deformation backward's buffers instead (include/fdgs.h)
        FDGS_REQUIRE(g->dL_dcolor && g->dL_dmeans2D && g->scratch_acc, "required gradient buffer is NULL");
    } else {
        FDGS_REQUIRE(g->dL_dcolor && g->dL_dmeans2D && g->dL_dmeans3D && g->dL_dopacity && g->dL_dcolors && g->dL_dcov3D &&
                         g->scratch_acc, "required gradient buffer is NULL");
        FDGS_REQUIRE(!p->shs || g->dL_dsh, "dL_dsh required when shs is given");
        FDGS_REQUIRE(p->cov3D_precomp || (g->dL_dscales && g->dL_drotations), "dL_dscales/dL_drotations required");
    }
    hipStream_t stream = (hipStream_t)stream_;
    const size_t P = (size_t)p->P;
    // the per-Gaussian outputs are written for every Gaussian by preprocess_bwd; only the atomic accumulator needs zeros
    if (!g->scratch_acc_zeroed) FDGS_HIP_CHECK(hipMemsetAsync(g->scratch_acc, 0, P * 64, stream));      // (1: the forward filled it, fdgs_raster_params::acc_zero)
    if (p->cov3D_precomp) {   // scale/rotation gradients do not exist on this path: hand back zeros if buffers were given
        if (g->dL_dscales) FDGS_HIP_CHECK(hipMemsetAsync(g->dL_dscales, 0, P * 12, stream));
        if (g->dL_drotations) FDGS_HIP_CHECK(hipMemsetAsync(g->dL_drotations, 0, P * 16, stream));
    }
    if (R > 0) {
        RenderBwdArgs a{};
        const ImgLayout il = fill_blend_args(a, p, geom, binning, img, R);
        a.dL_dcolor = g->dL_dcolor; a.dL_ddepth = g->dL_ddepth; a.dL_dalpha = dL_dalpha;
        a.gacc = g->scratch_acc;
        // (the order lists live in `img`, the forward's state, which this call otherwise only reads: the slice written here is scratch of the
        // backward that belongs to this frame -- one backward per forward state at a time, as for every other buffer of the state)
        a.order = make_tile_order(stream, 1, il, img, const_cast<void*>(img));
        {
            FDGS_TIMED("render_bwd", stream);
            // -1 (default): by image size -- one wave per tile leaves the chip underfilled when the image has fewer tiles than the chip has wave
            // slots (1 024 SIMDs x 4): two waves per tile then (config 3, 2 040 tiles: blending backward 0.274 -> 0.213 ms; config 2, 2 500
            // tiles: 0.197 -> 0.187; at 5 440 tiles four pixels per lane win by 10 %, profiles/r05_rbwd_ppl_small_images_ab.txt)
            launch_render_bwd(stream, g_tune.rbwd_ppl >= 0 ? g_tune.rbwd_ppl : (a.gx * a.gy <= 4096 ? 2 : 4), g->dL_ddepth != nullptr,
                              means2D_abs != nullptr, a);
        }
        FDGS_LAUNCH_CHECK("render_bwd", p->debug, stream);
    }
    return fdgs_launch_preprocess_bwd(stream, p, geom, g, antialiasing, means2D_abs);
}

extern "C" int fdgs_raster_bwd(void* stream_,const fdgs_raster_params* p, const void* geom, const void* binning,
                               const void* img, uint32_t R, const fdgs_raster_grads* g) {
    return raster_bwd_impl(stream_, p, geom, binning, img, R, g, nullptr);
}

extern "C" int fdgs_raster_bwd_alpha(void* stream_, const fdgs_raster_params* p, const void* geom, const void* binning,
                                     const void* img, uint32_t R, const fdgs_raster_grads* g, const float* dL_dalpha) {
    return raster_bwd_impl(stream_, p, geom, binning, img, R, g, dL_dalpha);
}

extern "C" int fdgs_raster_bwd_aa(void* stream_, const fdgs_raster_params* p, const void* geom, const void* binning,
                                  const void* img, uint32_t R, const fdgs_raster_grads* g, const float* dL_dalpha) {
    return raster_bwd_impl(stream_, p, geom, binning, img, R, g, dL_dalpha, true);
}

extern "C" int fdgs_raster_bwd_abs(void* stream_, const fdgs_raster_params* p, const void* geom, const void* binning, const void* img,
                                   uint32_t R, const fdgs_raster_grads* g, const float* dL_dalpha, int antialiased, float* dL_dmeans2D_abs) {
    return raster_bwd_impl(stream_, p, geom, binning, img, R, g, dL_dalpha, antialiased != 0, dL_dmeans2D_abs);
}
