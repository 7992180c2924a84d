// tile_walk.h -- device code of binning form 1 that more than one unit runs: the walk over a wave's (tile, Gaussian) pairs (the per-tile
// count of preprocess.hip and the count / emit of binning.hip), the LDS-privatised per-tile count built on it, and the scan of the counts
// into the tiles' ranges (binning.hip alone, render.hip in one grid with the forward's tile order).
#pragma once
#include "common.h"

namespace fdgs {

// The pairs of a Gaussian are the tiles of its square, under culling the set bits of its 256-bit mask (squares of more than 256 tiles are
// not culled): the pair set of expand_pairs_kernel.  walk_pairs() hands every pair of a wave's 64 Gaussians to `f`: a square of up to 64
// tiles is walked by its own lane (its mask is one 64-bit word: pop the lowest set bit), a larger one by the whole wave, 64 tiles per
// round (the nearest Gaussians cover 60+ tiles each: one lane would keep 63 waiting).  Must be called by all lanes of the wave.
template <typename F>
__device__ __forceinline__ void walk_pairs(uint32_t cnt, uint2 rc, uint4 mlo, uint4 mhi, bool culled, uint32_t gx, uint32_t gid, F f) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t xmin = rc.x & 0xFFFFu, ymin = rc.x >> 16, w = (rc.y & 0xFFFFu) - xmin, h = (rc.y >> 16) - ymin;
    const uint32_t area = cnt ? w * h : 0u;
    const bool masked = culled && area <= 256u;
    if (area != 0u && area <= 64u) {
        unsigned long long m = masked ? (((unsigned long long)mlo.y << 32) | mlo.x) : (area == 64u ? ~0ull : (1ull << area) - 1ull);
        const uint32_t inv = (65536u + w - 1u) / w;          // l / w = (l * inv) >> 16 for l < 64, w <= 64
        const uint32_t tile0 = ymin * gx + xmin;
        while (m) {
            const uint32_t l = (uint32_t)__ffsll((unsigned long long)m) - 1u;
            m &= m - 1ull;
            const uint32_t q = (l * inv) >> 16;
            f(tile0 + q * gx + (l - q * w), gid);
        }
    }
    uint64_t big = __ballot(area > 64u);
    while (big) {
        const int src = __ffsll((unsigned long long)big) - 1;
        big &= big - 1ull;
        const uint32_t brx = __shfl(rc.x, src, 64), bry = __shfl(rc.y, src, 64), bgid = __shfl(gid, src, 64);
        const uint32_t bx = brx & 0xFFFFu, by = brx >> 16, bw = (bry & 0xFFFFu) - bx, barea = bw * ((bry >> 16) - by);
        if (culled && barea <= 256u) {
            // bit l of the mask = 32-bit word l / 32, bit l % 32: round k looks at l = 64 k + lane
            const uint32_t w0 = __shfl(mlo.x, src, 64), w1 = __shfl(mlo.y, src, 64), w2 = __shfl(mlo.z, src, 64), w3 = __shfl(mlo.w, src, 64);
            const uint32_t w4 = __shfl(mhi.x, src, 64), w5 = __shfl(mhi.y, src, 64), w6 = __shfl(mhi.z, src, 64), w7 = __shfl(mhi.w, src, 64);
            const bool up = lane >= 32u;
            const uint32_t word[4] = {up ? w1 : w0, up ? w3 : w2, up ? w5 : w4, up ? w7 : w6};
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t l = 64u * k + lane;
                if (l < barea && ((word[k] >> (lane & 31u)) & 1u)) {
                    const uint32_t q = l / bw;
                    f((by + q) * gx + bx + (l - q * bw), bgid);
                }
            }
        } else {
            for (uint32_t l = lane; l < barea; l += 64u) {
                const uint32_t q = l / bw;
                f((by + q) * gx + bx + (l - q * bw), bgid);
            }
        }
    }
}

// The per-tile pair count of a workgroup's Gaussians (one per thread: its pair count `cnt`, square `rc` and mask): counters privatised in
// LDS (s_cnt[ntiles]; ds_add -- global atomics into a few hot cells run at 5 G/s), then ONE global atomic per touched tile onto
// gcount.  Reached by every thread of the workgroup; a workgroup with nothing on screen leaves before the sweeps over the counters, which
// are as wide as the workgroup.
__device__ __forceinline__ void count_tile_pairs(uint32_t* s_cnt, uint32_t cnt, uint2 rc, uint4 mlo, uint4 mhi, bool culled, uint32_t gx,
                                                 uint32_t ntiles, uint32_t* __restrict__ gcount) {
    if (!__syncthreads_or(cnt != 0u)) return;
    const uint32_t t = threadIdx.x;
    for (uint32_t k = t; k < ntiles; k += blockDim.x) s_cnt[k] = 0u;
    __syncthreads();
    walk_pairs(cnt, rc, mlo, mhi, culled, gx, 0u, [&](uint32_t tile, uint32_t) { atomicAdd(&s_cnt[tile], 1u); });
    __syncthreads();
    for (uint32_t k = t; k < ntiles; k += blockDim.x) {
        const uint32_t n = s_cnt[k];
        if (n) atomicAdd(&gcount[k], n);
    }
}

// Exclusive scan of the tiles' pair counts by ONE 1024-thread workgroup = the tiles' slot ranges, written as `ranges`; empty tiles get
// (0, 0).  `cap` (capacity mode): a tile whose range would end behind it gets (0, 0) too, and so does every tile after it (the ends never
// decrease): the frame keeps whole tiles, in image order, while they fit.  `cursor` (opt): cleared per tile, for an emit that claims its
// slots on a cursor of its own.  Up to 16 consecutive tiles per thread (ntiles <= 16 384): one round of loads, one scan over the threads.
__device__ __forceinline__ void tile_scan_body(uint32_t* wsum /* LDS [16] */, const uint32_t* __restrict__ cnt, uint32_t ntiles,
                                               uint2* __restrict__ ranges, uint32_t* __restrict__ cursor, uint32_t cap) {
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint32_t items = (ntiles + 1023u) >> 10, i0 = t * items;
    uint32_t v[16], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
        v[k] = (k < items && i0 + k < ntiles) ? cnt[i0 + k] : 0u;
        sum += v[k];
    }
    uint32_t inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(inc, o, 64);
        if (lane >= (uint32_t)o) inc += u;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t run = inc - sum;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) run += k < w ? wsum[k] : 0u;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
        if (k < items && i0 + k < ntiles) {
            const uint32_t end = run + v[k];
            ranges[i0 + k] = (v[k] == 0u || end > cap) ? make_uint2(0u, 0u) : make_uint2(run, end);
            if (cursor) cursor[i0 + k] = 0u;
            run = end;
        }
    }
}

}  // namespace fdgs
