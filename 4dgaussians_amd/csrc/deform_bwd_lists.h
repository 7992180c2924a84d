// deform_bwd_lists.h -- what runs in front of the backward's products: the prep kernel (packed gradient rows, identity paths) and the kernels
// that turn the per-tile flags into tile / row lists.  Included by deform.hip inside namespace fdgs, after the forward kernels.

// ------------------------------------------------------------------------------------------------ backward: prep
// Per Gaussian: activation Jacobians -> packed pre-activation output gradients G[n][64]; direct (identity) paths.
struct PrepArgs {
    int N, Npad, activate, dc_stride, rest_stride;
    const float *g_xyz, *g_scales, *g_rot, *g_opacity, *g_shs, *out_scales, *out_rot, *out_opacity, *rot_norm;
    float *d_xyz, *d_scales, *d_rot, *d_opacity, *d_shs_dc, *d_shs_rest;
    float* G;
    uint32_t* tile_live;   // [Npad/32]: bit r set when packed row r of the 32-row tile is non-zero
};
// One wave per 64 consecutive Gaussians.  Every array is written as one contiguous block per wave (G: 16 KB, d_shs:
// 12 KB, d_xyz: 768 B ...) by staging the per-Gaussian rows in LDS and walking the block linearly, lane-consecutive:
// the round-1 kernel wrote 4..16-byte pieces at 12..256-byte strides and rocprofv3 showed 2.1x write and 2.4x fetch
// amplification on it (profiles/r01c_pmc_*).
__global__ void __launch_bounds__(256) deform_bwd_prep_kernel(PrepArgs a) {
    __shared__ __attribute__((aligned(16))) float lds_all[4 * 64 * 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* small = lds_all + wave * 64 * 64;   // [64][16]: the 11 pre-activation gradients of the k<=4 heads (+ padding)
    float* sh = small + 64 * 16;               // [64][48]: g_shs rows
    const int n0 = (blockIdx.x * 4 + wave) * 64;
    if (n0 >= a.Npad) return;
    const int n = n0 + lane;
    const int nvalid = a.N - n0 < 64 ? (a.N - n0 > 0 ? a.N - n0 : 0) : 64;   // Gaussians of this wave that exist
    float row[16];
#pragma unroll
    for (int i = 0; i < 16; i++) row[i] = 0.f;
    if (n < a.N) {
        if (a.g_xyz) { row[0] = a.g_xyz[3 * (size_t)n]; row[1] = a.g_xyz[3 * (size_t)n + 1]; row[2] = a.g_xyz[3 * (size_t)n + 2]; }
        if (a.g_scales) {
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const float gs = a.g_scales[3 * (size_t)n + i];
                row[3 + i] = a.activate ? gs * a.out_scales[3 * (size_t)n + i] : gs;  // d exp
            }
        }
        if (a.g_rot) {
            const float4 gr = reinterpret_cast<const float4*>(a.g_rot)[n];
            if (a.activate) {
                const float4 o = reinterpret_cast<const float4*>(a.out_rot)[n];
                const float nrm = a.rot_norm[n];
                if (nrm > 1e-12f) {
                    const float dot = o.x * gr.x + o.y * gr.y + o.z * gr.z + o.w * gr.w;
                    const float inv = 1.0f / nrm;
                    row[6] = (gr.x - o.x * dot) * inv; row[7] = (gr.y - o.y * dot) * inv;
                    row[8] = (gr.z - o.z * dot) * inv; row[9] = (gr.w - o.w * dot) * inv;
                } else {  // below the F.normalize eps the division is by the constant 1e-12
                    row[6] = gr.x * 1e12f; row[7] = gr.y * 1e12f; row[8] = gr.z * 1e12f; row[9] = gr.w * 1e12f;
                }
            } else { row[6] = gr.x; row[7] = gr.y; row[8] = gr.z; row[9] = gr.w; }
        }
        if (a.g_opacity) {
            const float go = a.g_opacity[n];
            const float o = a.activate ? a.out_opacity[n] : 0.f;
            row[10] = a.activate ? go * o * (1.f - o) : go;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
        reinterpret_cast<float4*>(small)[lane * 4 + i] = make_float4(row[4 * i], row[4 * i + 1], row[4 * i + 2], row[4 * i + 3]);
    // g_shs block of this wave: [64][48] floats = 768 float4, contiguous in memory
    const float4* gsh4 = a.g_shs ? reinterpret_cast<const float4*>(a.g_shs + (size_t)n0 * 48) : nullptr;
#pragma unroll
    for (int j = 0; j < 12; j++) {
        const int v = j * 64 + lane;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gsh4 && v < nvalid * 12) x = gsh4[v];
        reinterpret_cast<float4*>(sh)[v] = x;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    // ---- per 32-row tile: does any row carry a gradient?  (the backward kernels skip tiles of all-zero rows)
    {
        bool nz = false;
#pragma unroll
        for (int i = 0; i < 11; i++) nz = nz || (row[i] != 0.f);
#pragma unroll
        for (int j = 0; j < 12; j++) {
            const float4 x = reinterpret_cast<const float4*>(sh)[lane * 12 + j];
            nz = nz || x.x != 0.f || x.y != 0.f || x.z != 0.f || x.w != 0.f;
        }
        const unsigned long long m = __ballot(nz);
        if (lane == 0) {
            a.tile_live[n0 >> 5] = (uint32_t)(m & 0xffffffffull);       // (bit r = row r of the tile is non-zero: the row lists are built from these)
            a.tile_live[(n0 >> 5) + 1] = (uint32_t)(m >> 32);
        }
    }
    // ---- packed gradient rows G[n][64] = [small 16 | shs 48] (padded rows n >= N are zero)
    {
        float4* G4 = reinterpret_cast<float4*>(a.G + (size_t)n0 * GCOLS);
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int v = j * 64 + lane, r = v >> 4, c4 = v & 15;
            G4[v] = c4 < 4 ? reinterpret_cast<const float4*>(small)[r * 4 + c4] : reinterpret_cast<const float4*>(sh)[r * 12 + (c4 - 4)];
        }
    }
    // ---- identity paths (out = in + delta): accumulate into the parameter gradients, block-linear
    if (a.d_shs_dc && a.d_shs_rest && a.dc_stride == 48 && a.rest_stride == 48 && a.d_shs_rest == a.d_shs_dc + 3) {
        float4* d4 = reinterpret_cast<float4*>(a.d_shs_dc + (size_t)n0 * 48);   // one combined [N,16,3] tensor
#pragma unroll
        for (int j = 0; j < 12; j++) {
            const int v = j * 64 + lane;
            if (v < nvalid * 12) {
                float4 x = d4[v];
                const float4 y = reinterpret_cast<const float4*>(sh)[v];
                x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
                d4[v] = x;
            }
        }
    } else {
        if (a.d_shs_dc) {
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const int idx = j * 64 + lane, r = idx / 3, c = idx - 3 * r;
                if (r < nvalid) a.d_shs_dc[(size_t)(n0 + r) * a.dc_stride + c] += sh[r * 48 + c];
            }
        }
        if (a.d_shs_rest) {
            for (int j = 0; j < 45; j++) {
                const int idx = j * 64 + lane, r = idx / 45, c = idx - 45 * r;
                if (r < nvalid) a.d_shs_rest[(size_t)(n0 + r) * a.rest_stride + c] += sh[r * 48 + 3 + c];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int idx = j * 64 + lane, r = idx / 3, c = idx - 3 * r;
        if (r < nvalid) {
            if (a.d_xyz) a.d_xyz[(size_t)n0 * 3 + idx] += small[r * 16 + c];
            if (a.d_scales) a.d_scales[(size_t)n0 * 3 + idx] += small[r * 16 + 3 + c];
        }
    }
    if (a.d_rot) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int idx = j * 64 + lane, r = idx >> 2, c = idx & 3;
            if (r < nvalid) a.d_rot[(size_t)n0 * 4 + idx] += small[r * 16 + 6 + c];
        }
    }
    if (a.d_opacity && lane < nvalid) a.d_opacity[n] += small[lane * 16 + 10];
}

// ------------------------------------------------------------------------------------------------ live-tile lists
// Lists written by an EARLIER kernel are read through the constant address space: a wave-uniform index then gives a scalar
// (s_load) read.  Through a plain global pointer the compiler must assume the kernel's own stores may alias the list and falls back
// to a vector load + readfirstlane -- which joins the in-order vmcnt queue behind the prefetched activation rows and drags the
// derived addresses into vector registers.
typedef const uint32_t __attribute__((address_space(4))) * const_u32p;
__device__ __forceinline__ const_u32p as_const(const uint32_t* p) { return (const_u32p)(unsigned long long)p; }

// The rasterizer hands zero gradient rows to every Gaussian that is culled, off-screen or fully occluded (on the bench scene:
// 88 % of them, profiles/r03a_zero_gradient_rows.jsonl), and a zero row adds exactly zero to every sum the backward forms.
// With the set in spatial order such Gaussians are contiguous, so whole 32-row tiles are zero: the packing stage
// (deform_bwd_prep_kernel, or fdgs_raster_bwd's epilogue) leaves one flag per tile behind, this kernel turns the flags into
//   live[]   : ascending indices of the tiles with a non-zero row, padded to a multiple of 4 with a zero tile (D2's workgroups take
//              four tiles at a time and meet at barriers),
//   chunks[] : ascending indices of the plane-gradient chunks (tpc tiles each) that contain a live tile,
//   counters : { live tiles, live tiles padded, live chunks, tiles },
// and D2 / D3 / D4 walk the lists instead of 0 .. Npad/32.  One workgroup; ~5 us.  skip = 0 lists every tile (A/B, FDGS_SKIP_DEAD=0).
struct CompactArgs {
    uint32_t* flags; uint32_t* live; uint32_t* chunks; uint32_t* counters;    // (skip = 0: flags are WRITTEN here, all ones)
    int ntiles, tpc, skip;
    float* G;      // packed rows: the dead tile used as padding of live[] gets zero rows here (its producer may have left them unwritten)
    // ROW lists (fdgs_tuning "row_compact", saved activations + spatially ordered input): rowbase[t] = live rows in front of tile t;
    // row_gather_kernel then lists the live rows (ascending) in rows[] and copies their packed gradient rows, in that order, to Gc;
    // this kernel pads both to a multiple of row_pad rows (pad entries: ROW_PAD | 0, zero gradient rows).  NULL: tile lists only.
    uint32_t* rowbase; uint32_t* rows; float* Gc;
    int row_pad;
};
constexpr uint32_t ROW_PAD = 0x80000000u;       // rows[] entry: padding (index bits = a valid row to read activations from, here 0)
__global__ void __launch_bounds__(1024) tile_compact_kernel(CompactArgs a) {
    __shared__ uint32_t wl[16], wc[16], wr[16];
    __shared__ uint32_t first_dead;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (t == 0) first_dead = 0xffffffffu;
    __syncthreads();
    int span = (a.ntiles + 1023) / 1024;
    span = (span + 3) & ~3;                              // (ntiles and span are multiples of 4: aligned uint4 reads, whole chunks)
    const int b = t * span, e = b + span < a.ntiles ? b + span : a.ntiles;
    uint32_t nl = 0, nc = 0, nr = 0, fd = 0xffffffffu;
    for (int i = b; i < e; i += 4) {
        uint4 f = make_uint4(1u, 1u, 1u, 1u);
        if (a.skip) f = reinterpret_cast<const uint4*>(a.flags)[i >> 2];
        // every tile is walked: D2 writes every tile's DFEAT rows, and the plane-gradient kernels (which mask DFEAT rows with these flags)
        // must see them all -- the flags may never have been written (packed_rows_ready = 1) or mark zero rows (harmless either way)
        else reinterpret_cast<uint4*>(a.flags)[i >> 2] = f;
        const uint32_t fv[4] = {f.x != 0u, f.y != 0u, f.z != 0u, f.w != 0u};
        nr += (uint32_t)(__popc(f.x) + __popc(f.y) + __popc(f.z) + __popc(f.w));
#pragma unroll
        for (int j = 0; j < 4; j++) {
            nl += fv[j];
            if (!fv[j] && fd == 0xffffffffu) fd = (uint32_t)(i + j);
        }
        if (a.tpc == 4) nc += (fv[0] | fv[1] | fv[2] | fv[3]);
        else if (a.tpc == 2) nc += (fv[0] | fv[1]) + (fv[2] | fv[3]);
        else nc += fv[0] + fv[1] + fv[2] + fv[3];
    }
    if (fd != 0xffffffffu) atomicMin(&first_dead, fd);
    uint32_t il = nl, ic = nc, ir = nr;       // inclusive scans inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t ul = __shfl_up(il, o, 64), uc = __shfl_up(ic, o, 64), ur = __shfl_up(ir, o, 64);
        if (lane >= o) { il += ul; ic += uc; ir += ur; }
    }
    if (lane == 63) { wl[wv] = il; wc[wv] = ic; wr[wv] = ir; }
    __syncthreads();
    uint32_t pl = il - nl, pc = ic - nc, pr = ir - nr, tl = 0, tc = 0, tr = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) {
        if (w < wv) { pl += wl[w]; pc += wc[w]; pr += wr[w]; }
        tl += wl[w]; tc += wc[w]; tr += wr[w];
    }
    for (int i = b; i < e; i += 4) {
        uint4 f = make_uint4(1u, 1u, 1u, 1u);
        if (a.skip) f = reinterpret_cast<const uint4*>(a.flags)[i >> 2];
        const uint32_t fv[4] = {f.x != 0u, f.y != 0u, f.z != 0u, f.w != 0u};
        if (a.rowbase) {
            const uint32_t c0 = (uint32_t)__popc(f.x), c1 = (uint32_t)__popc(f.y), c2 = (uint32_t)__popc(f.z);
            reinterpret_cast<uint4*>(a.rowbase)[i >> 2] = make_uint4(pr, pr + c0, pr + c0 + c1, pr + c0 + c1 + c2);
            pr += c0 + c1 + c2 + (uint32_t)__popc(f.w);
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (fv[j]) a.live[pl++] = (uint32_t)(i + j);
        if (a.tpc == 4) { if (fv[0] | fv[1] | fv[2] | fv[3]) a.chunks[pc++] = (uint32_t)(i >> 2); }
        else if (a.tpc == 2) { if (fv[0] | fv[1]) a.chunks[pc++] = (uint32_t)(i >> 1); if (fv[2] | fv[3]) a.chunks[pc++] = (uint32_t)((i >> 1) + 1); }
        else {
#pragma unroll
            for (int j = 0; j < 4; j++) if (fv[j]) a.chunks[pc++] = (uint32_t)(i + j);
        }
    }
    if (a.skip && a.G && (tl & 3u) != 0u && first_dead != 0xffffffffu) {
        float* rows = a.G + (size_t)first_dead * 32 * GCOLS;
        for (int k = t; k < 32 * GCOLS; k += 1024) rows[k] = 0.f;
    }
    // row lists: pad to whole units of row_pad rows (>= 128: D2's workgroups take four 32-row tiles at a time; D4 takes whole chunks)
    const uint32_t rp = a.rowbase ? (tr + (uint32_t)a.row_pad - 1u) / (uint32_t)a.row_pad * (uint32_t)a.row_pad : 0u;
    if (a.rowbase) {
        for (uint32_t k = tr + t; k < rp; k += 1024) a.rows[k] = ROW_PAD;
        float4* gz = reinterpret_cast<float4*>(a.Gc + (size_t)tr * GCOLS);
        for (uint32_t k = t; k < (rp - tr) * (GCOLS / 4); k += 1024) gz[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (t == 0) {
        const uint32_t n4 = (tl + 3u) & ~3u;
        // (tl % 4 != 0 implies a dead tile exists, because ntiles % 4 == 0)
        for (uint32_t k = tl; k < n4; k++) a.live[k] = first_dead;
        a.counters[0] = tl; a.counters[1] = n4; a.counters[2] = tc; a.counters[3] = (uint32_t)a.ntiles;
        // [4] live rows, [5] 32-row tiles of the padded row list, [6] plane-gradient chunks of it
        a.counters[4] = tr; a.counters[5] = rp / 32u; a.counters[6] = a.rowbase ? rp / (32u * (uint32_t)a.tpc) : 0u;
    }
}

// rows[] and the compact copy of the packed gradient rows.  One wave per 64 rows (two tiles); a wave without a live row returns at once.
struct RowGatherArgs { const uint32_t* flags; const uint32_t* rowbase; const float* G; uint32_t* rows; float* Gc; int ntiles; };
__global__ void __launch_bounds__(256) row_gather_kernel(RowGatherArgs a) {
    __shared__ uint8_t lst_all[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int t0 = (blockIdx.x * 4 + wv) * 2;           // first tile of this wave (ntiles is a multiple of 4)
    if (t0 >= a.ntiles) return;
    const uint32_t m0 = a.flags[t0], m1 = a.flags[t0 + 1];
    if ((m0 | m1) == 0u) return;
    const uint32_t b0 = a.rowbase[t0];                  // (rowbase[t0 + 1] = b0 + popc(m0): the wave's live rows are one run of the list)
    const unsigned long long m = (unsigned long long)m0 | ((unsigned long long)m1 << 32);
    const bool on = (m >> lane) & 1ull;
    const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    uint8_t* lst = lst_all[wv];
    if (on) { a.rows[b0 + rank] = (uint32_t)(t0 * 32 + lane); lst[rank] = (uint8_t)lane; }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    const int cnt = __popcll(m), sub = lane >> 4, c4 = lane & 15;    // four rows per pass: 16 lanes x 16 bytes each
    const float4* G4 = reinterpret_cast<const float4*>(a.G + (size_t)t0 * 32 * GCOLS);
    float4* O4 = reinterpret_cast<float4*>(a.Gc + (size_t)b0 * GCOLS);
    for (int e0 = 0; e0 < cnt; e0 += 4) {
        const int e = e0 + sub;
        if (e < cnt) O4[e * 16 + c4] = G4[(int)lst[e] * 16 + c4];
    }
}

// The same in ONE launch (no rowbase array, no tile_compact_kernel) for sets of up to ROW_LIST_MAX_TILES tiles: a workgroup owns 8 tiles
// (256 rows) and counts the live rows in front of them itself -- a sum over the row masks of the earlier tiles, at most 64 KB of
// coalesced reads, skipped by the workgroups without a live row (80 % on the bench scene) -- then lists and copies like row_gather_kernel.
// The workgroup of the last tiles also leaves the counters and the padding (what tile_compact_kernel does in the two-launch form).
constexpr int ROW_LIST_MAX_TILES = 16384;
struct RowListArgs { const uint32_t* flags; const float* G; uint32_t* rows; float* Gc; uint32_t* counters; int ntiles, tpc, row_pad; };
__global__ void __launch_bounds__(256) row_list_kernel(RowListArgs a) {
    __shared__ uint8_t lst_all[4][64];
    __shared__ uint32_t s_part[4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int tb = blockIdx.x * 8;                      // first tile of this workgroup (ntiles is a multiple of 4)
    const bool last = tb + 8 >= a.ntiles;
    const int t0 = tb + 2 * wv;                         // first tile of this wave
    const uint32_t m0 = t0 < a.ntiles ? a.flags[t0] : 0u, m1 = t0 + 1 < a.ntiles ? a.flags[t0 + 1] : 0u;
    const int wcnt = __popc(m0) + __popc(m1);
    if (!last && __syncthreads_or(wcnt) == 0) return;   // (uniform: a workgroup of dead tiles has nothing to list)
    uint32_t part = 0;
    for (int i = t; i < tb; i += 256) part += (uint32_t)__popc(a.flags[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    if (lane == 0) s_part[wv] = part;
    __syncthreads();
    const uint32_t base = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    __syncthreads();
    if (lane == 0) s_part[wv] = (uint32_t)wcnt;
    __syncthreads();
    uint32_t b0 = base;
    for (int w = 0; w < wv; w++) b0 += s_part[w];
    if (wcnt) {
        const unsigned long long m = (unsigned long long)m0 | ((unsigned long long)m1 << 32);
        const bool on = (m >> lane) & 1ull;
        const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        uint8_t* lst = lst_all[wv];
        if (on) { a.rows[b0 + rank] = (uint32_t)(t0 * 32 + lane); lst[rank] = (uint8_t)lane; }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        const int sub = lane >> 4, c4 = lane & 15;      // four rows per pass: 16 lanes x 16 bytes each
        const float4* G4 = reinterpret_cast<const float4*>(a.G + (size_t)t0 * 32 * GCOLS);
        float4* O4 = reinterpret_cast<float4*>(a.Gc + (size_t)b0 * GCOLS);
        for (int e0 = 0; e0 < wcnt; e0 += 4) {
            const int e = e0 + sub;
            if (e < wcnt) O4[e * 16 + c4] = G4[(int)lst[e] * 16 + c4];
        }
    }
    if (last) {      // totals, padding to whole units of row_pad rows, counters (the tile lists are not built: nobody reads them in this form)
        const uint32_t tr = base + s_part[0] + s_part[1] + s_part[2] + s_part[3];
        const uint32_t rp = (tr + (uint32_t)a.row_pad - 1u) / (uint32_t)a.row_pad * (uint32_t)a.row_pad;
        for (uint32_t k = tr + t; k < rp; k += 256) a.rows[k] = ROW_PAD;
        float4* gz = reinterpret_cast<float4*>(a.Gc + (size_t)tr * GCOLS);
        for (uint32_t k = t; k < (rp - tr) * (GCOLS / 4); k += 256) gz[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t == 0) {
            a.counters[0] = 0u; a.counters[1] = 0u; a.counters[2] = 0u; a.counters[3] = (uint32_t)a.ntiles;
            a.counters[4] = tr; a.counters[5] = rp / 32u; a.counters[6] = rp / (32u * (uint32_t)a.tpc);
        }
    }
}
