// blend_replay.h -- the replay walk: what the kernels share that walk the lists of a FINISHED frame once more with the forward's own
// decisions (render_pick_kernel, render_features_kernel, render_contrib_kernel in render.hip; render_features_bwd_kernel in
// render_features_bwd.h).  Included by render.hip inside namespace fdgs, behind blend_power* and BlendHead.
//
// The walk ("replay walk"): one 256-thread workgroup per tile, in the forward's own tile order (read, never rebuilt); the
// tile's list goes through LDS in rounds of 256 entries -- recA, recB and where needed the ids; recC is not read --, ids two rounds ahead
// and records one round ahead in registers; every lane walks up to its pixel's n_contrib and the workgroup leaves once every lane is
// through (`__syncthreads_count(seen >= mine) == 256`).  Each kernel keeps its own round loop (its staging differs, and a loop behind a
// callback left a per-lane object in memory); the pieces of it are here.  Everything is compiled without contraction.  Nothing of the
// frame is written by any of these kernels.
#pragma once

struct ReplayArgs : BlendHead {
    const uint32_t* tile_todo;               // per tile: max n_contrib, the forward's walk length
    const uint2* ranges; const uint32_t* pair_gid;
    const float4 *recA, *recB;
    const uint32_t* n_contrib;
    uint32_t R; int P;                       // what the lists were laid out for: fences for a stale img
    int empty;                               // 1: no Gaussians or no pairs, nothing of the frame is read (the pick and feature passes still
                                             // write every pixel; the contribution pass and the adjoint are not launched)
};
// (EMPTY, below: the kernel may be launched on an empty frame.  A template bool, not a second struct: the two kernels that never are lose
// some hundred instructions of prologue with it, and the adjoint 0.5 % of its time.)

// the block's tile (< 0: none, leave) and the thread's pixel of it; `own`: the pixel's n_contrib, 0 outside the image or on an empty frame
struct ReplayPixel {
    int tile, x, y;
    bool inside;
    float pxf, pyf;
    size_t pix;
    uint32_t own;
};
template <bool EMPTY>
__device__ __forceinline__ ReplayPixel replay_pixel(const ReplayArgs& a) {
    ReplayPixel p;
    const int t = threadIdx.x;
    const bool empty = EMPTY && a.empty;
    p.tile = empty ? unit_of_block(blockIdx.x, a.gx, a.gy, 1, a.bh) : unit_lookup(a.order, a.per_xcd, blockIdx.x, a.gx, a.gy, 1, a.bh);
    if (p.tile >= a.gx * a.gy) p.tile = -1;
    p.x = (p.tile % a.gx) * TILE + (t & 15); p.y = (p.tile / a.gx) * TILE + (t >> 4);
    p.inside = p.tile >= 0 && p.x < a.W && p.y < a.H;
    p.pxf = (float)p.x; p.pyf = (float)p.y;
    p.pix = (size_t)p.y * a.W + p.x;
    p.own = p.inside && !empty ? a.n_contrib[p.pix] : 0u;
    return p;
}

// The tile's list, clamped to what the lists were laid out for, and how far it is walked: `todo` by the tile (the forward's tile_todo,
// clamped to the list), `mine` = min(own, todo) by this lane, `rounds` of 256 staged entries.  `own` is the caller's: the contribution pass
// zeroes it where the pixel does not count.  ONE rule for the four kernels; the pick kernel used to clamp a lane to the list, min(own,
// n_list).  For any frame the forward wrote own <= tile_todo[tile], so the two are equal; the clamp to todo is what keeps a lane inside
// the rounds the workgroup stages when img is stale.
struct ReplayLengths {
    uint2 range;
    int n_list, todo, mine, rounds;
};
template <bool EMPTY>
__device__ __forceinline__ ReplayLengths replay_lengths(const ReplayArgs& a, int tile, uint32_t own) {
    ReplayLengths l;
    l.range = make_uint2(0u, 0u);
    uint32_t walk = 0u;
    if (!(EMPTY && a.empty)) {
        l.range = a.ranges[tile];
        l.range.y = l.range.y < a.R ? l.range.y : a.R;
        l.range.x = l.range.x < l.range.y ? l.range.x : l.range.y;
        walk = a.tile_todo[tile];
    }
    l.n_list = (int)(l.range.y - l.range.x);
    l.todo = walk < (uint32_t)l.n_list ? (int)walk : l.n_list;
    l.mine = own < (uint32_t)l.todo ? (int)own : l.todo;
    l.rounds = (l.todo + 255) / 256;
    return l;
}

// the id this thread stages in round r (behind the end of the list: a copy of its last entry, never walked)
__device__ __forceinline__ uint32_t replay_gid(const ReplayArgs& a, const ReplayLengths& l, int r) {
    const int e = r * 256 + (int)threadIdx.x;
    return a.pair_gid[l.range.x + (e < l.n_list ? e : l.n_list - 1)];
}

// the longest walk among the wave's 64 pixels: the kernels that reduce over the wave per entry run every lane that far
__device__ __forceinline__ int replay_wave_mine(int mine) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int u = __shfl_xor(mine, o, 64); mine = u > mine ? u : mine; }
    return mine;
}

// THE FORWARD'S DECISION about one staged entry (A, B = its recA, recB) at the pixel (pxf, pyf) with transmittance T in front of it, in
// render_fwd_kernel's own expressions (the original; that kernel contracts only its colour sums, which do not exist here): the exponent
// and alpha, each written once ...
__device__ __forceinline__ float replay_power(const float4 A, const float4 B, float pxf, float pyf) {
#pragma clang fp contract(off)
    const float dx = A.x - pxf, dy = A.y - pyf;
    return blend_power(blend_power_xx(A.z, dx), blend_power_xy(A.w, dx), B.x, dy);
}
__device__ __forceinline__ float replay_alpha(const float4 B, float power) {
#pragma clang fp contract(off)
    return fminf(FDGS_ALPHA_MAX, B.y * __expf(power));
}
// ... and the forward's two skips with what it did to an entry it kept: the blend weight w = alpha * T -- on its bits -- and the
// transmittance behind the entry, T (1 - alpha).  (Its third decision, T (1 - alpha) < 1e-4, ends a pixel's walk: the replay stops at
// n_contrib instead.)  Every bitwise test of the replay passes rests on these bodies.  The rule stands twice, side by side and nowhere
// else, because the kernels need it compiled in two shapes and the compiler takes the shape from the source:
//   replay_weight  hands back values, w = 0 for a skipped entry: the second skip becomes a select.  What the adjoint and the contribution
//                  pass were compiled to when the rule stood in them (the adjoint with branches: 88 VGPRs for 72, five waves per SIMD
//                  for six; so does a helper CALL on the kept path, which is why w and T are spelled out in both).
//   replay_hit     runs on_hit(w, T behind) for a kept entry and nothing for a skipped one: both skips stay branches around a long kept
//                  path.  What the pick and the feature pass were compiled to (with the select the pick kernel ran 11 % longer).
struct ReplayWeight {
    float w, T;
};
__device__ __forceinline__ ReplayWeight replay_weight(const float4 A, const float4 B, float pxf, float pyf, float T) {
#pragma clang fp contract(off)
    const float power = replay_power(A, B, pxf, pyf);
    if (power > 0.0f) return {0.0f, T};
    const float alpha = replay_alpha(B, power);
    if (alpha < FDGS_ALPHA_MIN) return {0.0f, T};
    return {alpha * T, T * (1.0f - alpha)};
}
template <typename F>
__device__ __forceinline__ void replay_hit(const float4 A, const float4 B, float pxf, float pyf, float T, F&& on_hit) {
#pragma clang fp contract(off)
    const float power = replay_power(A, B, pxf, pyf);
    if (power > 0.0f) return;
    const float alpha = replay_alpha(B, power);
    if (alpha < FDGS_ALPHA_MIN) return;
    on_hit(alpha * T, T * (1.0f - alpha));
}

// the caller's row of Gaussian g: g itself or row_map[g], -1 where g is no Gaussian of the frame (>= P: a stale list) or the row is not
// below `bound` (a -1 of the map is not below any bound)
__device__ __forceinline__ int32_t replay_row(const ReplayArgs& a, uint32_t g, const int32_t* row_map, uint32_t bound) {
    if (g >= (uint32_t)a.P) return -1;
    const uint32_t row = row_map ? (uint32_t)row_map[g] : g;
    return row < bound ? (int32_t)row : -1;
}
