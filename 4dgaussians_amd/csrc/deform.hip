// deform.hip -- D1..D4: fused HexPlane + deformation-MLP forward and backward for gfx950.
//
// Replaces, per frame, the ~60 unfused PyTorch launches of scene/hexplane.py:73-106 (6*L grid_sample + product +
// concat), scene/deformation.py:67-83,97-148 (trunk Linear + five 2-layer heads, out = in + delta) and the
// activations of gaussian_renderer/__init__.py:97-99.
//
// Layout of the MLP on the matrix cores (exact-f32 v_mfma_f32_32x32x2_f32, so results equal an fmaf chain):
//   * one wave64 owns 32 Gaussians; lane = (g = lane&31, h = lane>>5);
//   * every layer is computed TRANSPOSED, D[feature][gaussian] = W[feature][k] * X[k][gaussian]: the weight matrix is
//     the A operand (row-major [out][in] as torch stores it -> contiguous float4 loads along k, no repacking) and the
//     activations are the B operand;
//   * the MFMA C/D layout puts row (reg&3)+8*(reg>>2)+4*h of column g into lane (g,h) register reg -- which is
//     exactly the B-operand layout of the NEXT layer if its k-steps are walked in that row order.  So activations
//     never leave registers between layers (hidden layers use the "interleaved" tile layout described at the MFMA
//     layer helpers below, which makes W X and W^T dY both read the weights with 16-byte loads).
//   D1 forward: gather features (channel-last planes, one float4 = 4 channels per corner), trunk, heads (k <= 4 outputs on
//      the 4x4x1 MFMA), epilogue; optionally parks features / relu(hidden) / relu(h1) for the backward ("saved").
//   D2 backward-data (persistent, one workgroup per CU): per 32-Gaussian tile and head -- the relu(h1) tile (copied from
//      the saved activations, or recomputed), dW2/db2 (register sums for the k <= 4 heads, column ownership over the
//      workgroup's four tiles for the 48-row SH head), dh1 = W2^T G, dhid += W1^T dh1; then dfeat = W0^T dhid.  Writes
//      dH1 / dHidden (/ relu(hidden) / features when recomputing) for the weight-gradient GEMM.
//   D3 weight gradients: dW = dY^T X with K = #Gaussians; one wave owns a whole [W x W] product for its slice, one 16-byte
//      load per operand per 16 MFMAs, LDS reduction over the workgroup, one coalesced atomic flush per workgroup.
//   D4 plane gradients: lanes <-> (x-corner, channel) so that every float atomic instruction covers whole texel lines
//      (scattered float atomics run at only ~20 G line-ops/s on MI355X: profiles/r01_atomic_microbench.txt); the three
//      time planes are privatised in LDS.
//   Round 3: the backward kernels walk only the 32-Gaussian tiles that carry a non-zero gradient row (tile_compact_kernel turns the
//      rasterizer backward's per-tile flags into lists: culled / occluded Gaussians add exactly zero to every sum); D1 deals the tiles left
//      over after the last full round of its persistent loop out by head (FDGS_D1_SPLIT).
// This file is the host side only: validation, the layouts of the caller's buffers, one launch plan per pass and the C ABI.  The kernels are
// the headers included below: deform_layers.h (MFMA wrappers, HexPlane sampling, DeformDev, the dense-layer blocks), deform_fwd32.h / _fwd16.h /
// _fwd_ws.h (D1, three forms), hexplane_ops.h (the index arithmetic of the HexPlane lookup, host/device, contraction off), deform_bwd_lists.h (prep, tile / row lists), deform_bwd32.h / _bwd_ws.h (D2), deform_wgrad.h (D3), deform_plane_grad.h (D4), deform_time_grad.h (dL/dt behind a finished backward: fdgs_deform_time_grad, opt-in).
// Knobs (development / A-B only; the table is in api.hip, the struct in common.h, the defaults are the tuned values): d1_form, d1_wgs,
// d1_split, skip_dead, row_compact, d2_form, d4_mfma, d4_rows_kb.  Build flags: -DFDGS_PROFILE_D1 / _WS / _D2 / _D2WS / _D4 add an in-kernel
// s_memtime phase profile of one kernel (printed once to stderr); -DFDGS_DEV_ONLY_44 builds only the (128, 32) instance.
#include "common.h"
#include "hexplane_ops.h"

#include <vector>

namespace fdgs {

#include "deform_layers.h"
#include "deform_fwd32.h"
#include "deform_fwd16.h"
#include "deform_fwd_ws.h"
#include "deform_bwd_lists.h"
#include "deform_bwd32.h"
#include "deform_bwd_ws.h"
#include "deform_wgrad.h"
#include "deform_plane_grad.h"
#include "deform_time_grad.h"

// ------------------------------------------------------------------------------------------------ host side
static int validate_deform(const fdgs_deform_params* p) {
    FDGS_REQUIRE(p != nullptr, "params is NULL");
    FDGS_REQUIRE(p->N >= 0, "N < 0");
    FDGS_REQUIRE(p->C == 16 || p->C == 32, "output_coordinate_dim must be 16 or 32");
    FDGS_REQUIRE(p->L >= 1 && p->L <= FDGS_MAX_LEVELS, "1 <= len(multires) <= 4");
    FDGS_REQUIRE(p->W == 64 || p->W == 128, "net_width must be 64 or 128");
    const int F = p->C * p->L;
    FDGS_REQUIRE(F <= 128, "C*L must be <= 128");
    for (int l = 0; l < p->L; l++) {
        for (int k = 0; k < 6; k++) FDGS_REQUIRE(p->planes[l][k] != nullptr, "plane pointer is NULL");
        for (int i = 0; i < 4; i++) FDGS_REQUIRE(p->res[l][i] >= 2 && p->res[l][i] <= 4096, "plane resolution must be in [2, 4096]");
        for (int k = 0; k < 6; k++) {
            const int a = k < 3 ? 0 : (k < 5 ? 1 : 2), b = k < 3 ? k + 1 : (k < 5 ? k - 1 : 3);
            FDGS_REQUIRE((long long)p->res[l][a] * p->res[l][b] * p->C * 4 < (1ll << 31), "plane larger than 2 GiB");
        }
    }
    FDGS_REQUIRE(p->w0 && p->b0, "trunk weights missing");
    for (int hd = 0; hd < FDGS_NUM_HEADS; hd++)
        if (p->head_on[hd]) FDGS_REQUIRE(p->w1[hd] && p->b1[hd] && p->w2[hd] && p->b2[hd], "head weights missing");
    if (p->N > 0) FDGS_REQUIRE(p->xyz && p->scales && p->rotations && p->opacity && p->shs_dc && p->shs_rest, "input pointer missing");
    for (int i = 0; i < 3; i++) FDGS_REQUIRE(p->aabb[3 + i] != p->aabb[i], "degenerate aabb");
    FDGS_REQUIRE(p->shs_dc_stride >= 3 && p->shs_rest_stride >= 45, "shs strides too small");
    return FDGS_OK;
}

template <template <int, int> class Launcher, typename Arg>
static int dispatch_wf(int W, int F, hipStream_t stream, int blocks, const Arg& arg) {
#define FDGS_CASE(WT_, FCH_) \
    if (W == WT_ * 32 && F == FCH_ * 8) { Launcher<WT_, FCH_>::go(stream, blocks, arg); return FDGS_OK; }
#ifdef FDGS_DEV_ONLY_44   // development builds: only the (net_width 128, C*L 32) instance, for quick ISA inspection
    FDGS_CASE(4, 4)
#else
    FDGS_CASE(2, 4) FDGS_CASE(2, 6) FDGS_CASE(2, 8) FDGS_CASE(2, 12) FDGS_CASE(2, 16)
    FDGS_CASE(4, 4) FDGS_CASE(4, 6) FDGS_CASE(4, 8) FDGS_CASE(4, 12) FDGS_CASE(4, 16)
#endif
#undef FDGS_CASE
    return fail(FDGS_E_INVALID, "%s", "unsupported (net_width, C*L) combination");
}

static size_t npad_of(int N) { return ((size_t)(N > 0 ? N : 1) + 127) / 128 * 128; }
static unsigned head_mask_of(const fdgs_deform_params* p) {
    unsigned m = 0u;
    for (int hd = 0; hd < FDGS_NUM_HEADS; hd++) m |= p->head_on[hd] ? 1u << hd : 0u;
    return m;
}
static int active_heads(const fdgs_deform_params* p) { return __builtin_popcount(head_mask_of(p)); }
// position of each active head in the per-head arrays (saved relu(h1), DH1)
static void head_slots(const fdgs_deform_params* p, int* slot_of) {
    int slot = 0;
    for (int hd = 0; hd < FDGS_NUM_HEADS; hd++) slot_of[hd] = p->head_on[hd] ? slot++ : 0;
}

// Which (WT = net_width / 32, FCH = C*L / 8) have an instance of the weight-stationary / the 16-Gaussian forward: the one rule behind the
// run-time choice (plan_fwd) and the launchers' if constexpr.  Both need C*L % 16 == 0; net_width 128 with C*L > 48 has no weight-stationary
// instance: W0 no longer fits the registers next to the five W1 -- and that kernel must not spill.
constexpr bool has_fwd_ws(int WT, int FCH) { return FCH % 2 == 0 && (WT == 2 || (WT == 4 && FCH <= 6)); }
constexpr bool has_fwd16(int /*WT*/, int FCH) { return FCH % 2 == 0; }

template <int WT, int FCH>
struct FwdWsLauncher {
    static void go(hipStream_t s, int blocks, const DeformDev& d) {
        if constexpr (has_fwd_ws(WT, FCH)) {
            constexpr int RT = WT / 2;
            const bool save = d.sv_h1 != nullptr, allh = d.head_mask == 31u;
            if (save && allh) hipLaunchKernelGGL((deform_mlp_ws_kernel<RT, FCH / 2, true, true>), dim3(blocks), dim3(256), 0, s, d);
            else if (save) hipLaunchKernelGGL((deform_mlp_ws_kernel<RT, FCH / 2, true, false>), dim3(blocks), dim3(256), 0, s, d);
            else if (allh) hipLaunchKernelGGL((deform_mlp_ws_kernel<RT, FCH / 2, false, true>), dim3(blocks), dim3(256), 0, s, d);
            else hipLaunchKernelGGL((deform_mlp_ws_kernel<RT, FCH / 2, false, false>), dim3(blocks), dim3(256), 0, s, d);
        } else {
            // never runs (plan_fwd asks has_fwd_ws too) and launches nothing.  The mention alone keeps these three 32-Gaussian instances where
            // they have always been in the code object -- kernels are emitted in order of first use -- so that a build can be compared with
            // its predecessor byte for byte; it goes with the next change to the device code.
            (void)&deform_fwd_kernel<WT, FCH>;
        }
    }
};
template <int WT, int FCH>
struct Fwd16Launcher {
    static void go(hipStream_t s, int blocks, const DeformDev& d) {
        if constexpr (has_fwd16(WT, FCH)) hipLaunchKernelGGL((deform_fwd16_kernel<2 * WT, FCH / 2>), dim3(blocks), dim3(256), 0, s, d);
    }
};
template <int WT, int FCH>
struct FwdLauncher {
    static void go(hipStream_t s, int blocks, const DeformDev& d) {
        hipLaunchKernelGGL((deform_fwd_kernel<WT, FCH>), dim3(blocks), dim3(256), 0, s, d);
    }
};
template <int WT, int FCH, bool SAVED, bool ROWS = false>
static void launch_bwd_data(hipStream_t s, int max_blocks, const BwdDev& d) {
    // persistent: as many workgroups as are co-resident (each keeps dW2/db2 sums in LDS), tiles handed out round-robin
    static int resident_of[FDGS_MAX_DEVICES] = {};
    int& resident = resident_of[current_device_slot()];
    if (resident == 0) {
        int per_cu = 1;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, deform_bwd_data_kernel<WT, FCH, SAVED, ROWS>, 256, 0) != hipSuccess || per_cu < 1)
            per_cu = 1;
        resident = device_cus() * per_cu;
    }
    int blocks = resident;
    if (blocks > max_blocks) blocks = max_blocks;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL((deform_bwd_data_kernel<WT, FCH, SAVED, ROWS>), dim3(blocks), dim3(256), 0, s, d);
}
template <int WT, int FCH>
struct BwdLauncher {
    static void go(hipStream_t s, int max_blocks, const BwdDev& d) {
        // the weight-stationary form (deform_bwd_ws.h) where it applies: row lists, net_width 128, C*L in {32, 48}, all five heads (dynerf) or the
        // three of position / scale / rotation (hypernerf, dnerf)
        if constexpr (WT == 4 && (FCH % 2) == 0 && FCH <= 6) {
            const int mask = (int)head_mask_of(&d.p);
            if (d.sv_h1 && d.s.rows && (mask == 31 || mask == 7) && g_tune.d2_form != 32) {
                int blocks = device_cus();
                if (blocks > max_blocks * 8) blocks = max_blocks * 8;      // (never more workgroups than 16-row tiles)
                if (mask == 31) hipLaunchKernelGGL((deform_bwd_data_ws_kernel<FCH / 2, 31>), dim3(blocks), dim3(256), 0, s, d);
                else hipLaunchKernelGGL((deform_bwd_data_ws_kernel<FCH / 2, 7>), dim3(blocks), dim3(256), 0, s, d);
                return;
            }
        }
        if (d.sv_h1 && d.s.rows) launch_bwd_data<WT, FCH, true, true>(s, max_blocks, d);
        else if (d.sv_h1) launch_bwd_data<WT, FCH, true>(s, max_blocks, d);
        else launch_bwd_data<WT, FCH, false>(s, max_blocks, d);
    }
};

// activations the forward can leave behind for the backward (float offsets into the `saved` buffer)
struct SavedLayout { size_t Np, feat, rh, h1, hmask, floats; };
static SavedLayout saved_layout(const fdgs_deform_params* p) {
    SavedLayout s;
    s.Np = npad_of(p->N);
    const size_t F = (size_t)p->C * p->L, W = p->W;
    s.feat = 0; s.rh = s.feat + s.Np * F; s.h1 = s.rh + s.Np * W;
    s.hmask = s.h1 + s.Np * W * active_heads(p);
    s.floats = s.hmask + s.Np * 8;   // 64 lanes x 4 words per 32 Gaussians
    return s;
}

// scratch of fdgs_deform_bwd (float offsets): the packed gradient rows, DIRECTLY followed by the per-tile flags (the layout
// include/fdgs.h promises to fdgs_raster_bwd's epilogue), the lists built from them, then the inter-kernel arrays
struct BwdLayout { size_t G, flags, live, chunks, counters, DH1, DHID, RH, FEAT, DFEAT, rowbase, rows, Gc, floats; };
static BwdLayout bwd_layout(const fdgs_deform_params* p) {
    BwdLayout b;
    const size_t Np = npad_of(p->N), F = (size_t)p->C * p->L, W = p->W, nt = Np / 32;
    size_t o = 0;
    auto take = [&](size_t n) { const size_t r = o; o = (o + n + 63) / 64 * 64; return r; };
    b.G = take(Np * GCOLS); b.flags = take(nt); b.live = take(nt + 4); b.chunks = take(nt); b.counters = take(64);
    b.DH1 = take(Np * W * (size_t)active_heads(p)); b.DHID = take(Np * W); b.RH = take(Np * W); b.FEAT = take(Np * F); b.DFEAT = take(Np * F);
    // row-list form (behind everything the older layout promised): live rows in front of each tile, the list, the compact copy of G
    b.rowbase = take(nt); b.rows = take(Np + 256); b.Gc = take((Np + 256) * GCOLS);
    b.floats = o;
    return b;
}

#if defined(FDGS_PROFILE_D1) || defined(FDGS_PROFILE_WS) || defined(FDGS_PROFILE_D2) || defined(FDGS_PROFILE_D2WS) || defined(FDGS_PROFILE_D4)
// In-kernel phase profiles (development builds only).  A profiled kernel adds its s_memtime counters into `n` zeroed 64-bit words.  A Run
// around a launch zeroes them and hands them to the kernel's argument; the launch after `after` earlier ones (past the warm-up) is waited for
// and given to `print`, once.
struct PhaseProfile {
    size_t n; int after; void (*print)(const unsigned long long*);
    unsigned long long* dev = nullptr; int calls = 0;
    struct Run {
        PhaseProfile& p; hipStream_t stream;
        Run(PhaseProfile& p_, hipStream_t stream_, unsigned long long** arg) : p(p_), stream(stream_) {
            if (!p.dev) (void)hipMalloc(&p.dev, p.n * sizeof(unsigned long long));
            (void)hipMemsetAsync(p.dev, 0, p.n * sizeof(unsigned long long), stream);
            *arg = p.dev;
        }
        ~Run() {
            if (p.calls++ != p.after) return;
            std::vector<unsigned long long> hb(p.n);
            (void)hipStreamSynchronize(stream);
            (void)hipMemcpy(hb.data(), p.dev, p.n * sizeof(unsigned long long), hipMemcpyDeviceToHost);
            p.print(hb.data());
        }
    };
};
// the common report: hb[i] = ticks of phase i summed over the waves, hb[8] = waves; `head` is the label line (takes the wave count)
static void print_phase_table(const char* head, const char* const* names, int n, int width, const unsigned long long* hb) {
    const double waves = (double)(hb[8] ? hb[8] : 1);
    double tot = 0;
    for (int i = 0; i < n; i++) tot += (double)hb[i];
    fprintf(stderr, head, hb[8]);
    for (int i = 0; i < n; i++) fprintf(stderr, "  %-*s %12.0f  (%.1f %%)\n", width, names[i], (double)hb[i] / waves, 100.0 * hb[i] / tot);
}
static void print_d1_profile(const unsigned long long* hb) {
#ifdef FDGS_PROFILE_WS
    const char* ws[7] = {"(loop top)", "feature park + request", "barrier", "copy-out + hmask", "heads", "epilogue", "trunk of the next tile"};
    print_phase_table("[D1-ws profile] %llu waves, s_memtime ticks per wave:\n", ws, 7, 28, hb);
#endif
#ifdef FDGS_PROFILE_D1
    const char* names[8] = {"prologue (query, inputs, preloads)", "gather", "feat store + trunk + relu + park + hmask", "L1.run (+drains)",
                            "relu + park + next preloads", "L2 (+L2b)", "epilogue", "final drain"};
    print_phase_table("[D1 profile] %llu waves, cycles per wave:\n", names, 8, 44, hb);
    if (hb[9] || hb[10]) fprintf(stderr, "  of which: ring commit vmcnt(0) %.0f, s_barrier %.0f\n", (double)hb[9] / (double)hb[8], (double)hb[10] / (double)hb[8]);
#endif
}
static void print_d2ws_profile(const unsigned long long* hb) {
    const char* names[8] = {"loop edge", "wait + barrier 1", "ReLU bits, DMA issue, first head's slots", "product 4 (no riders)", "xp write",
                            "product 0 (+ head 1, exchange A)", "product 1 (+ head 2, exchange B, barrier 2)", "products 2, 3 (+ head 3, exchange C; + SH head)"};
    print_phase_table("[D2-ws profile] %llu waves, s_memtime ticks per wave (100 MHz):\n", names, 8, 44, hb);
}
constexpr size_t D2_PROF_WAVES = 4096, D4_PROF_WGS = 64;     // (records of 12 words per wave / 16 x 10 words per workgroup, 8 waves used)
static void print_d2_profile(const unsigned long long* hb) {
    double sum[12] = {0}; int waves = 0;
    for (size_t w = 0; w < D2_PROF_WAVES; w++) {
        if (hb[w * 12 + 9] == 0) continue;
        waves++;
        for (int i = 0; i < 12; i++) sum[i] += (double)hb[w * 12 + i];
    }
    const char* names[12] = {"saved: head top .. rows in LDS", "saved: SH barrier wait", "recompute: L1.run | saved: masks + next-row requests",
                             "operand preloads", "dW2 small heads (+ pre-barrier)", "dh1", "mask+DH1 store", "B1.run", "tail(DHID,B0,DFEAT)",
                             "wave total", "saved: SH cooperative block", "saved: SH requests after the block"};
    fprintf(stderr, "[D2 profile] %d waves, s_memtime ticks (100 MHz) per wave:\n", waves);
    for (int i = 0; i < 12; i++) fprintf(stderr, "  %-26s %12.0f  (%.1f %%)\n", names[i], sum[i] / waves, 100.0 * sum[i] / sum[9]);
}
static void print_d4_profile(const unsigned long long* hb) {
    const char* nm[8] = {"S0+bar", "S", "bar(S)", "M.sp.loop", "M.sp.flush", "M.time", "bar(M)", "dxyz+bar"};
    for (int wv : {0, 1, 2, 3, 5, 6, 7}) {
        double sum[10] = {0}; int cnt = 0;
        for (size_t b = 0; b < D4_PROF_WGS; b++) { const unsigned long long* r = &hb[(b * 8 + wv) * 10]; if (!r[9]) continue; cnt++; for (int i = 0; i < 10; i++) sum[i] += (double)r[i]; }
        if (!cnt) continue;
        fprintf(stderr, "[D4 profile] wave %2d (total %.0f cyc, s_memtime units):", wv, sum[9] / cnt);
        for (int i = 0; i < 8; i++) fprintf(stderr, " %s %.1f%%", nm[i], 100.0 * sum[i] / sum[9]);
        fprintf(stderr, "\n");
    }
}
#endif

// ---- the forward's launch plan: which form of D1 runs, the grid of its gather and its workgroups
// Forms (g_tune.d1_form forces one where it has an instance; 0 = by shape):
//    8  weight-stationary (deform_fwd_ws.h; the gather is a kernel of its own in front of it and needs somewhere to put the features: the saved
//       activations or the pack scratch).  By shape at net_width 128 with up to two HexPlane levels: the gather kernel's time grows with the
//       levels while form 16 hides its gather under its products (profiles/r06_d1_forms_by_config.txt: config 3, three levels: 0.432 + 0.062 ms
//       against 0.462 + 0.006; configs 4 / 5, two levels: 0.570 + 0.039 against 0.633, 3.70 + 0.21 against 4.11); config 2 (net_width 64)
//       has a 0.8-ms frame paced by the host, where one more launch costs more than the kernel gains.
//   16  two waves per SIMD on packed operand streams (deform_fwd16.h; needs the pack scratch).  By shape everywhere else: in the frame, where
//       the gather starts on cold caches behind the previous frame's backward, it measured 5 - 7 % faster than form 32 on every workload
//       (profiles/r04_d1_forms.txt).
//   32  deform_fwd32.h: also what runs when the caller hands over no scratch.
// (validate_deform has made C 16 or 32, so C*L is a multiple of 16 and every lane group of forms 8 / 16 owns whole float4 texel quarters.)
// Workgroups: persistent, one (form 32; form 8 at net_width 128) or two (form 16; form 8 at net_width 64) per CU, never more than there are
// 128-Gaussian (form 8: 16-Gaussian) units of work.  d1_wgs > 0 sets the number; 0 = one workgroup per unit (forms 16 / 32: not persistent).
struct FwdPlan { int form; dim3 gather_grid; int wgs; };
static FwdPlan plan_fwd(const fdgs_deform_params* p, const fdgs_deform_out* out, int Npad) {
    const int WT = p->W / 32, FCH = p->C * p->L / 8, want_form = g_tune.d1_form, cus = device_cus();
    FwdPlan pl{};
    if ((want_form == 8 || (want_form == 0 && p->L <= 2 && p->W == 128)) && has_fwd_ws(WT, FCH) && (out->saved || out->packed)) pl.form = 8;
    else if (want_form != 32 && has_fwd16(WT, FCH) && out->packed) pl.form = 16;
    else pl.form = 32;
    if (pl.form == 8) {
        pl.gather_grid = dim3(cdiv((long long)Npad * (p->C / 4), 256), p->L);
        const int want = g_tune.d1_wgs > 0 ? g_tune.d1_wgs : (p->W == 128 ? 1 : 2) * cus, nt16 = Npad / 16;
        pl.wgs = want < nt16 ? want : nt16;
    } else {
        const int want = g_tune.d1_wgs >= 0 ? g_tune.d1_wgs : (pl.form == 16 ? 2 : 1) * cus;
        const int units = 4 * cdiv(p->N, 128) / (pl.form == 16 ? 2 : 4);     // (form 16: four 16-Gaussian tiles per workgroup)
        pl.wgs = want > 0 && want < units ? want : units;
    }
    return pl;
}

// the forward kernel of the planned form (timed alone; the gather / the operand-stream copy in front of it have their own rows)
static int launch_fwd(hipStream_t stream, const FwdPlan& plan, DeformDev& d) {
    d.prof = nullptr;
#if defined(FDGS_PROFILE_D1) || defined(FDGS_PROFILE_WS)
    static PhaseProfile prof{16, 5, print_d1_profile};
    PhaseProfile::Run run(prof, stream, &d.prof);
#endif
    int rc;
    {
        FDGS_TIMED("deform_fwd", stream);
        rc = plan.form == 8 ? dispatch_wf<FwdWsLauncher>(d.p.W, d.F, stream, plan.wgs, d)
           : plan.form == 16 ? dispatch_wf<Fwd16Launcher>(d.p.W, d.F, stream, plan.wgs, d) : dispatch_wf<FwdLauncher>(d.p.W, d.F, stream, plan.wgs, d);
    }
    if (rc) return rc;
    FDGS_LAUNCH_CHECK("deform_fwd", 0, stream);
    return FDGS_OK;
}

// ---- the backward's steps, in launch order.  Each returns its status; fdgs_deform_bwd below is their sequence.
static BwdScratch bwd_scratch(const fdgs_deform_params* p, float* base, const BwdLayout& bl) {
    BwdScratch s;
    s.Npad = (int)npad_of(p->N);
    s.G = base + bl.G; s.DH1 = base + bl.DH1; s.DHID = base + bl.DHID; s.RH = base + bl.RH; s.FEAT = base + bl.FEAT; s.DFEAT = base + bl.DFEAT;
    s.tile_live = reinterpret_cast<uint32_t*>(base + bl.flags); s.live = reinterpret_cast<uint32_t*>(base + bl.live);
    s.chunks = reinterpret_cast<uint32_t*>(base + bl.chunks); s.counters = reinterpret_cast<uint32_t*>(base + bl.counters);
    s.rows = nullptr;
    return s;
}

// prep: activation Jacobians, identity paths, packed gradient rows
static int bwd_prep(hipStream_t stream, const fdgs_deform_params* p, const fdgs_deform_grads* g, const BwdScratch& s) {
    PrepArgs pa{};
    pa.N = p->N; pa.Npad = s.Npad; pa.activate = p->activate; pa.dc_stride = p->shs_dc_stride; pa.rest_stride = p->shs_rest_stride;
    pa.g_xyz = g->g_xyz; pa.g_scales = g->g_scales; pa.g_rot = g->g_rotations; pa.g_opacity = g->g_opacity; pa.g_shs = g->g_shs;
    pa.out_scales = g->out_scales; pa.out_rot = g->out_rotations; pa.out_opacity = g->out_opacity; pa.rot_norm = g->rot_norm;
    pa.d_xyz = g->d_xyz; pa.d_scales = g->d_scales; pa.d_rot = g->d_rotations; pa.d_opacity = g->d_opacity;
    pa.d_shs_dc = g->d_shs_dc; pa.d_shs_rest = g->d_shs_rest; pa.G = s.G; pa.tile_live = s.tile_live;
    { FDGS_TIMED("deform_bwd_prep", stream); hipLaunchKernelGGL(deform_bwd_prep_kernel, dim3(cdiv(s.Npad, 256)), dim3(256), 0, stream, pa); }
    FDGS_LAUNCH_CHECK("deform_bwd_prep", 0, stream);
    return FDGS_OK;
}

// What the backward walks, decided on the host from (p, g, the knobs) alone: fdgs_deform_bwd builds its lists by this plan, and
// fdgs_deform_time_grad / fdgs_deform_time_grad_dfeat, which read that call's scratch afterwards, find DFEAT by the same plan.
//   splat    the plane-gradient kernel: the matrix-core form (default whenever one frame time is shared by all Gaussians, i.e. on the render()
//            path; d4_mfma = 1 / 0 forces a kernel (A/B, tests), otherwise the caller's order hint decides), else the per-corner atomics
//   Gc       Gaussians per chunk of the splat (the chunk list is built for it)
//   skip     packed_rows_ready = 1: rows without flags -- every tile is live and the kernel writes the flags (all ones); 3: the rows of dead
//            tiles were never written -- skipping is not a choice then, whatever the A/B knob says
//   by_rows  ROW lists instead of tile lists: D2 / D3 / D4 walk only the rows that carry a gradient (on the bench scene 12 % of the rows, but
//            17.5 % of the 32-row tiles and 21 % of the 128-row chunks, are live).  Needs the saved activations (fetched row by row) and the
//            splat form of D4 (which takes its chunks from any list); the dead tiles must be skippable at all (flags present).
struct BwdListPlan { bool splat; int Gc; int skip; bool by_rows; };
static BwdListPlan plan_bwd_lists(const fdgs_deform_params* p, const fdgs_deform_grads* g) {
    BwdListPlan pl;
    pl.splat = !p->time && (g_tune.d4_mfma >= 0 ? g_tune.d4_mfma != 0 : g->spatially_ordered != 0);
    pl.Gc = 2048 / p->C;
    pl.skip = g->packed_rows_ready == 3 ? 1 : ((g_tune.skip_dead != 0 && g->packed_rows_ready != 1) ? 1 : 0);
    pl.by_rows = g_tune.row_compact != 0 && pl.skip && g->saved && pl.splat;
    return pl;
}

// tiles with a non-zero gradient row -> lists.  Leaves s.rows / s.G on the row list and the compact copy of G when the row form runs.
static int bwd_lists(hipStream_t stream, float* base, const BwdLayout& bl, const BwdListPlan& plan, BwdScratch& s) {
    const int Gc = plan.Gc;
    const bool by_rows = plan.by_rows;
    CompactArgs ca{};
    ca.flags = s.tile_live; ca.live = s.live; ca.chunks = s.chunks; ca.counters = s.counters; ca.G = s.G;
    ca.ntiles = s.Npad / 32; ca.tpc = Gc / 32;
    ca.skip = plan.skip;
    if (by_rows) {
        ca.rowbase = reinterpret_cast<uint32_t*>(base + bl.rowbase); ca.rows = reinterpret_cast<uint32_t*>(base + bl.rows); ca.Gc = base + bl.Gc;
        ca.row_pad = Gc > 128 ? Gc : 128;
    }
    const bool one_launch = by_rows && ca.ntiles <= ROW_LIST_MAX_TILES && g_tune.row_compact != 2;     // (knob value 2: the two-launch form at any size, tests)
    if (one_launch) {
        RowListArgs ra{};
        ra.flags = s.tile_live; ra.G = s.G; ra.rows = ca.rows; ra.Gc = ca.Gc; ra.counters = s.counters; ra.ntiles = ca.ntiles; ra.tpc = ca.tpc; ra.row_pad = ca.row_pad;
        { FDGS_TIMED("row_list", stream); hipLaunchKernelGGL(row_list_kernel, dim3(cdiv(ca.ntiles, 8)), dim3(256), 0, stream, ra); }
        FDGS_LAUNCH_CHECK("row_list", 0, stream);
    } else {
        { FDGS_TIMED("tile_compact", stream); hipLaunchKernelGGL(tile_compact_kernel, dim3(1), dim3(1024), 0, stream, ca); }
        FDGS_LAUNCH_CHECK("tile_compact", 0, stream);
        if (by_rows) {
            RowGatherArgs ra{};
            ra.flags = s.tile_live; ra.rowbase = ca.rowbase; ra.G = s.G; ra.rows = ca.rows; ra.Gc = ca.Gc; ra.ntiles = ca.ntiles;
            { FDGS_TIMED("row_gather", stream); hipLaunchKernelGGL(row_gather_kernel, dim3(cdiv(ca.ntiles, 8)), dim3(256), 0, stream, ra); }
            FDGS_LAUNCH_CHECK("row_gather", 0, stream);
        }
    }
    if (by_rows) { s.rows = ca.rows; s.G = ca.Gc; }       // (from here on "G" is the compact copy)
    return FDGS_OK;
}

static int bwd_data(hipStream_t stream, const fdgs_deform_params* p, const fdgs_deform_grads* g, const BwdScratch& s) {
    BwdDev bd;
    bd.p = *p; bd.sc = aabb_scale(p); bd.s = s; bd.F = p->C * p->L; bd.ntiles = s.Npad / 32; bd.small_heads = 1;
    bd.sv_rh = bd.sv_h1 = nullptr; bd.sv_hmask = nullptr;
    if (g->saved) {
        const SavedLayout sl = saved_layout(p);
        const float* sv = reinterpret_cast<const float*>(g->saved);
        bd.sv_rh = sv + sl.rh; bd.sv_h1 = sv + sl.h1; bd.sv_hmask = reinterpret_cast<const uint32_t*>(sv + sl.hmask);
    }
    head_slots(p, bd.head_slot);
    for (int hd = 0; hd < FDGS_NUM_HEADS; hd++) { bd.d_w2[hd] = g->d_w2[hd]; bd.d_b2[hd] = g->d_b2[hd]; }
    bd.prof = nullptr;
#ifdef FDGS_PROFILE_D2
    static PhaseProfile prof{D2_PROF_WAVES * 12, 5, print_d2_profile};
    PhaseProfile::Run run(prof, stream, &bd.prof);
#endif
#ifdef FDGS_PROFILE_D2WS
    static PhaseProfile prof_ws{16, 5, print_d2ws_profile};
    PhaseProfile::Run run_ws(prof_ws, stream, &bd.prof);
#endif
    int rc;
    {
        FDGS_TIMED("deform_bwd_data", stream);
        rc = dispatch_wf<BwdLauncher>(p->W, bd.F, stream, s.Npad / 128, bd);
    }
    if (rc) return rc;
    FDGS_LAUNCH_CHECK("deform_bwd_data", 0, stream);
    return FDGS_OK;
}

// weight gradients: one job per active head (dW1, db1) + the trunk (dW0, db0)
static int bwd_wgrad(hipStream_t stream, const fdgs_deform_params* p, const fdgs_deform_grads* g, const BwdScratch& s) {
    const size_t Np = (size_t)s.Npad;
    const int F = p->C * p->L, W = p->W;
    const float *X_rh = s.RH, *X_feat = s.FEAT;      // operands of the GEMMs: recomputed into the scratch by backward-data, or saved by the forward
    if (g->saved) {
        const SavedLayout sl = saved_layout(p);
        X_rh = reinterpret_cast<const float*>(g->saved) + sl.rh; X_feat = reinterpret_cast<const float*>(g->saved) + sl.feat;
    }
    WgradArgs wa{};
    wa.Npad = s.Npad; wa.W = W; wa.live = s.live; wa.counters = s.counters; wa.rows = s.rows;
    int nj = 0;
    for (int hd = 0; hd < FDGS_NUM_HEADS; hd++) {
        if (!p->head_on[hd]) continue;
        WgradJob& J = wa.job[nj++];
        J.DY = s.DH1 + (size_t)(nj - 1) * Np * W;      /* (a head's slab = its rank among the active heads) */ J.X = X_rh; J.dW = g->d_w1[hd]; J.db = g->d_b1[hd];
        J.ldx = W; J.ncols = W; J.ldw = W;
    }
    {
        WgradJob& J = wa.job[nj++];
        J.DY = s.DHID; J.X = X_feat; J.dW = g->d_w0; J.db = g->d_b0; J.ldx = F; J.ncols = F; J.ldw = F;
    }
    wa.njobs = nj;
    // one workgroup per CU; workgroups are shared out in proportion to the MFMA work of each job
    const int total_wgs = device_cus();
    int work[FDGS_NUM_HEADS + 1], total_work = 0;
    // cost model: MFMAs per k-step; the narrow trunk product (dword loads, only CT MFMAs per load pair, deep ring) is
    // memory-latency rather than MFMA bound: it costs about twice its MFMA count (sweep: 0.53 / 0.44 / 0.46 / 0.48 ms at
    // factor 1 / 2 / 3 / 4)
    const int trunk_factor = 2;
    for (int j = 0; j < nj; j++) {
        work[j] = (wa.job[j].ncols + 31) / 32;
        if (wa.job[j].ncols != W) work[j] *= trunk_factor;
        total_work += work[j];
    }
    // floor shares: never more workgroups than CUs (a single straggler would double the kernel time)
    int nbs[FDGS_NUM_HEADS + 1], used = 0;
    for (int j = 0; j < nj; j++) { nbs[j] = (int)((long long)total_wgs * work[j] / total_work); if (nbs[j] < 1) nbs[j] = 1; used += nbs[j]; }
    for (int j = 0; used < total_wgs; j = (j + 1) % nj) { nbs[j]++; used++; }   // leftovers round-robin, heads first
    int first = 0;
    const int ntl = s.Npad / 32;
    for (int j = 0; j < nj; j++) {
        WgradJob& J = wa.job[j];
        int nb = nbs[j];
        if (nb > ntl) nb = ntl;             // (never more workgroups than tiles)
        J.first_block = first; J.nblocks = nb;
        first += nb;
    }
    {
        FDGS_TIMED("deform_wgrad", stream);
        if (W == 128 && wa.rows) hipLaunchKernelGGL((deform_wgrad_kernel<4, true>), dim3(first), dim3(256), 0, stream, wa);
        else if (W == 128) hipLaunchKernelGGL((deform_wgrad_kernel<4, false>), dim3(first), dim3(256), 0, stream, wa);
        else if (wa.rows) hipLaunchKernelGGL((deform_wgrad_kernel<2, true>), dim3(first), dim3(256), 0, stream, wa);
        else hipLaunchKernelGGL((deform_wgrad_kernel<2, false>), dim3(first), dim3(256), 0, stream, wa);
    }
    FDGS_LAUNCH_CHECK("deform_wgrad", 0, stream);
    return FDGS_OK;
}

// LDS of the matrix-core splat (float offsets): the privatised time rows in front, then the dv tile, coordinates, axis descriptors and the rest
struct SplatLds { int dv, q, desc, dq, org, row, floats; };
static SplatLds splat_lds(int Gc, int C, int time_floats) {
    SplatLds m;
    int o = (time_floats + 63) / 64 * 64;
    auto take = [&](int n) { const int r = o; o += n; return r; };
    m.dv = take(6 * Gc * C); m.q = take(3 * Gc); m.desc = take(13 * Gc);   // (desc: [3][G] float4 axis descriptors + [G] window masks)
    m.dq = take(3 * Gc); m.org = take(96 + 9 * Gc); m.row = take(Gc);
    m.floats = o;
    return m;
}
#ifndef FDGS_D4_WGS
#define FDGS_D4_WGS 256
#endif
// either plane-gradient kernel.  `raise`: its dynamic-LDS limit (a function attribute, set per device) goes up to the CU's 160 KB before the
// device's first launch
template <typename Args>
static int launch_plane_grad(hipStream_t stream, void (*kernel)(Args), bool raise, bool* raised /*[FDGS_MAX_DEVICES]*/, int blocks, int threads,
                             size_t lds_bytes, const Args& a) {
    const void* fn = reinterpret_cast<const void*>(kernel);
    bool& r = raised[current_device_slot()];
    if (raise && !r) {
        FDGS_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        r = true;
    }
    { FDGS_TIMED("deform_plane_grad", stream); hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds_bytes, stream, a); }
    FDGS_LAUNCH_CHECK("deform_plane_grad", 0, stream);
    return FDGS_OK;
}

// plane + coordinate gradients.  splat: the matrix-core form, else the per-corner atomics (plan_bwd_lists)
static int bwd_plane_grads(hipStream_t stream, const fdgs_deform_params* p, const fdgs_deform_grads* g, const BwdScratch& s, bool splat, int Gc) {
    bool any_plane = g->d_xyz != nullptr;
    PlaneGradArgs ga{};
    ga.p = *p; ga.sc = aabb_scale(p); ga.DFEAT = s.DFEAT; ga.d_xyz = g->d_xyz; ga.F = p->C * p->L; ga.tile_live = s.tile_live;
    for (int l = 0; l < p->L; l++)
        for (int k = 0; k < 6; k++) { ga.d_planes[l][k] = g->d_planes[l][k]; any_plane = any_plane || g->d_planes[l][k]; }
    if (!any_plane) return FDGS_OK;
    // LDS privatisation of the time planes (one frame time for all Gaussians): greedy by level while the tiles fit.  Splat: the time rows
    // get what its fixed part (splat_lds, + 64 floats for the rows' padding) leaves of the CU's LDS, or d4_rows_kb if that is less (tests:
    // time rows that do not fit take the global-atomic path).  Per-corner form: up to 128 KB (one 512-thread workgroup per CU then; the
    // un-privatised alternative, float atomics on ~128 hot lines, is 4x slower than scattered atomics)
    int lds_budget = splat ? 160 * 1024 - (splat_lds(Gc, p->C, 0).floats + 64) * 4 : 128 * 1024;
    if (splat && g_tune.d4_rows_kb >= 0 && g_tune.d4_rows_kb * 1024 < lds_budget) lds_budget = g_tune.d4_rows_kb * 1024;
    int used = 0;
    for (int l = 0; l < FDGS_MAX_LEVELS; l++)
        for (int sl = 0; sl < 3; sl++) ga.lds_off[l][sl] = -1;
    if (!p->time) {
        for (int l = 0; l < p->L; l++) {
            int need = 0;
            for (int sl = 0; sl < 3; sl++) need += p->res[l][sl] * p->C;
            const int kk[3] = {2, 4, 5};
            bool wanted = true;
            for (int sl = 0; sl < 3; sl++) wanted = wanted && g->d_planes[l][kk[sl]];
            if (!wanted || (size_t)(used + need) * 4 > (size_t)lds_budget) continue;
            for (int sl = 0; sl < 3; sl++) { ga.lds_off[l][sl] = used; used += p->res[l][sl] * p->C; }
        }
    }
    ga.lds_floats = used;
    static bool raised[2][2][FDGS_MAX_DEVICES] = {};      // [kernel][C == 32][device]
    if (splat) {
        // workgroup shape of the splat: 8 waves, one workgroup per CU (4-wave workgroups with half the chunk, two per CU, measured equal on
        // BASELINE config 4 -- 0.331 vs 0.322 ms -- and were dropped)
        const SplatLds m = splat_lds(Gc, p->C, used);
        PlaneGradMArgs ma{};
        ma.g = ga;
        ma.prof = nullptr;
        ma.chunks = s.chunks; ma.counters = s.counters; ma.rows = s.rows;
        ma.off_dv = m.dv; ma.off_q = m.q; ma.off_desc = m.desc; ma.off_dq = m.dq; ma.off_org = m.org; ma.off_row = m.row;
        const int nchunks_max = cdiv(p->N, Gc), blocks = FDGS_D4_WGS < nchunks_max ? FDGS_D4_WGS : nchunks_max;
#ifdef FDGS_PROFILE_D4
        static PhaseProfile prof{D4_PROF_WGS * 16 * 10, 5, print_d4_profile};
        PhaseProfile::Run run(prof, stream, &ma.prof);
#endif
        return launch_plane_grad(stream, p->C == 16 ? deform_plane_grad_mfma_kernel<16, 8> : deform_plane_grad_mfma_kernel<32, 8>, true,
                                 raised[0][p->C == 32], blocks, 512, (size_t)m.floats * 4, ma);
    }
    const int gpb = (PG_THREADS / 64) * (64 / (2 * p->C));       // Gaussians per workgroup iteration
    const int nwg = 512;                                          // ~2 workgroups per CU
    int per_block = cdiv(cdiv(p->N, nwg), gpb) * gpb;
    if (per_block < gpb) per_block = gpb;
    ga.per_block = per_block;
    const int blocks = cdiv(p->N, per_block);
    const size_t lds_bytes = (size_t)used * 4;      // (above 64 KB, the default dynamic-LDS limit, the kernel has to opt in)
    return launch_plane_grad(stream, p->C == 16 ? deform_plane_grad_kernel<16> : deform_plane_grad_kernel<32>, lds_bytes > 64 * 1024,
                             raised[1][p->C == 32], blocks, PG_THREADS, lds_bytes, ga);
}

// ------------------------------------------------------------------------------------------------ probe of the HexPlane index arithmetic
struct CellsArgs { fdgs_deform_params p; AabbScale sc; int32_t* cells; float *w1, *dscale, *q; };
// one thread per Gaussian, plain vector stores; never on the frame path (tests/test_gpu_hexplane_cells.py compares it with the host twin)
__global__ void __launch_bounds__(256) hexplane_cells_kernel(CellsArgs a) {
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= a.p.N) return;
    const size_t per = (size_t)a.p.L * 4;
    hexplane_cells_row(a.p, a.sc.inv2, (size_t)n, a.cells + (size_t)n * per * 2, a.w1 + (size_t)n * per, a.dscale + (size_t)n * per, a.q + (size_t)n * 4);
}
static int validate_cells(const fdgs_deform_params* p, const void* cells, const void* w1, const void* dscale, const void* q) {
    FDGS_REQUIRE(p != nullptr, "params is NULL");
    FDGS_REQUIRE(p->N >= 0, "N < 0");
    FDGS_REQUIRE(p->L >= 1 && p->L <= FDGS_MAX_LEVELS, "1 <= len(multires) <= 4");
    for (int l = 0; l < p->L; l++)
        for (int i = 0; i < 4; i++) FDGS_REQUIRE(p->res[l][i] >= 2 && p->res[l][i] <= 4096, "plane resolution must be in [2, 4096]");
    for (int i = 0; i < 3; i++) FDGS_REQUIRE(p->aabb[3 + i] != p->aabb[i], "degenerate aabb");
    if (p->N > 0) FDGS_REQUIRE(p->xyz && cells && w1 && dscale && q, "NULL pointer");
    return FDGS_OK;
}

}  // namespace fdgs

using namespace fdgs;

extern "C" int fdgs_deform_fwd(void* stream_, const fdgs_deform_params* p, const fdgs_deform_out* out) {
    int rc = validate_deform(p);
    if (rc) return rc;
    FDGS_REQUIRE(out && (p->N == 0 || (out->xyz && out->scales && out->rotations && out->opacity && out->shs)), "output pointer missing");
    if (p->N == 0) return FDGS_OK;
    hipStream_t stream = (hipStream_t)stream_;
    DeformDev d;
    d.p = *p; d.out = *out; d.F = p->C * p->L; d.small_heads = 1; d.split_tail = g_tune.d1_split; d.sc = aabb_scale(p);
    const SavedLayout sl = saved_layout(p);
    float* sv = reinterpret_cast<float*>(out->saved);
    d.sv_feat = sv ? sv + sl.feat : nullptr; d.sv_rh = sv ? sv + sl.rh : nullptr; d.sv_h1 = sv ? sv + sl.h1 : nullptr;
    d.sv_hmask = sv ? reinterpret_cast<uint32_t*>(sv + sl.hmask) : nullptr;
    d.Npad = (int)sl.Np;
    head_slots(p, d.head_slot);
    d.ntiles = 4 * cdiv(p->N, 128);
    d.packed = reinterpret_cast<const float*>(out->packed);
    d.feat = nullptr;
    d.head_mask = head_mask_of(p);
    d.skew = 600;       // (s_memtime ticks; sweep 0 .. 24 k in profiles/r04_d1_forms.txt)
    const FwdPlan plan = plan_fwd(p, out, d.Npad);
    if (plan.form == 8) {
        // features: into the saved activations when the backward will want them, into the scratch otherwise
        GatherArgs ga{};
        ga.p = *p; ga.sc = d.sc; ga.F = d.F; ga.Npad = d.Npad; ga.feat = d.sv_feat ? d.sv_feat : reinterpret_cast<float*>(out->packed);
        d.feat = ga.feat;
        FDGS_TIMED("deform_gather", stream);
        hipLaunchKernelGGL(deform_gather_kernel, plan.gather_grid, dim3(256), 0, stream, ga);
    }
    if (plan.form == 16) {
        FDGS_TIMED("pack_weights", stream);
        PackArgs pa{};
        pa.w0 = p->w0; pa.W = p->W; pa.F = d.F; pa.out = reinterpret_cast<float*>(out->packed);
        for (int hd = 0; hd < FDGS_NUM_HEADS; hd++) { pa.w1[hd] = p->w1[hd]; pa.head_on[hd] = p->head_on[hd]; }
        const int n4 = (d.F * p->W + FDGS_NUM_HEADS * p->W * p->W) / 4;
        hipLaunchKernelGGL(pack_weights16_kernel, dim3(cdiv(n4, 256)), dim3(256), 0, stream, pa);
    }
    return launch_fwd(stream, plan, d);
}

extern "C" int fdgs_deform_pack_bytes(const fdgs_deform_params* p, size_t* bytes) {
    int rc = validate_deform(p);
    if (rc) return rc;
    FDGS_REQUIRE(bytes, "bytes is NULL");
    // the operand streams of the 16-Gaussian form, or -- weight-stationary form without saved activations -- the gathered features [Npad][C*L]
    const size_t streams = ((size_t)p->C * p->L * p->W + (size_t)FDGS_NUM_HEADS * p->W * p->W) * sizeof(float);
    const size_t feats = npad_of(p->N) * (size_t)p->C * p->L * sizeof(float);
    *bytes = streams > feats ? streams : feats;
    return FDGS_OK;
}

extern "C" int fdgs_deform_saved_bytes(const fdgs_deform_params* p, size_t* bytes) {
    int rc = validate_deform(p);
    if (rc) return rc;
    FDGS_REQUIRE(bytes, "bytes is NULL");
    *bytes = saved_layout(p).floats * sizeof(float) + 256;
    return FDGS_OK;
}

extern "C" int fdgs_deform_bwd_scratch_bytes(const fdgs_deform_params* p, size_t* bytes) {
    int rc = validate_deform(p);
    if (rc) return rc;
    FDGS_REQUIRE(bytes, "bytes is NULL");
    *bytes = bwd_layout(p).floats * sizeof(float) + 1024;
    return FDGS_OK;
}

extern "C" int fdgs_deform_bwd_live_tiles(void* stream_, const fdgs_deform_params* p, const void* scratch, uint32_t* out_host) {
    int rc = validate_deform(p);
    if (rc) return rc;
    FDGS_REQUIRE(scratch && out_host, "NULL pointer");
    const BwdLayout bl = bwd_layout(p);
    uint32_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    FDGS_HIP_CHECK(hipMemcpyAsync(c, reinterpret_cast<const float*>(scratch) + bl.counters, sizeof(c), hipMemcpyDeviceToHost, (hipStream_t)stream_));
    FDGS_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream_));
    // (row-list form: the 32-row units / chunks of the padded ROW list are what the kernels walked)
    out_host[0] = c[5] ? c[5] : c[1]; out_host[1] = c[3]; out_host[2] = c[5] ? c[6] : c[2];
    out_host[3] = (c[3] + 3) / 4;     // (reported in 128-Gaussian units)
    return FDGS_OK;
}

extern "C" int fdgs_deform_bwd(void* stream_, const fdgs_deform_params* p, const fdgs_deform_grads* g) {
    int rc = validate_deform(p);
    if (rc) return rc;
    FDGS_REQUIRE(g && g->scratch, "grads/scratch is NULL");
    if (p->N == 0) return FDGS_OK;
    if (p->activate && !g->packed_rows_ready) {
        FDGS_REQUIRE(!g->g_scales || g->out_scales, "out_scales needed with activate=1");
        FDGS_REQUIRE(!g->g_rotations || (g->out_rotations && g->rot_norm), "out_rotations/rot_norm needed with activate=1");
        FDGS_REQUIRE(!g->g_opacity || g->out_opacity, "out_opacity needed with activate=1");
    }
    hipStream_t stream = (hipStream_t)stream_;
    float* base = reinterpret_cast<float*>(g->scratch);
    const BwdLayout bl = bwd_layout(p);
    BwdScratch s = bwd_scratch(p, base, bl);
    if (!g->packed_rows_ready && (rc = bwd_prep(stream, p, g, s))) return rc;    // (1: fdgs_raster_bwd's deformation epilogue already wrote G and the identity paths)
    if (active_heads(p) == 0) return FDGS_OK;  // no head active: the deformation is the identity
    const BwdListPlan plan = plan_bwd_lists(p, g);
    if ((rc = bwd_lists(stream, base, bl, plan, s))) return rc;
    for (int hd = 0; hd < FDGS_NUM_HEADS; hd++)
        if (p->head_on[hd]) FDGS_REQUIRE(g->d_w1[hd] && g->d_b1[hd] && g->d_w2[hd] && g->d_b2[hd], "head gradient buffer missing");
    FDGS_REQUIRE(g->d_w0 && g->d_b0, "trunk gradient buffer missing");
    if ((rc = bwd_data(stream, p, g, s))) return rc;
    if ((rc = bwd_wgrad(stream, p, g, s))) return rc;
    return bwd_plane_grads(stream, p, g, s, plan.splat, plan.Gc);
}

// ---- dL/dt behind a finished backward (deform_time_grad.h).  The three entry points find DFEAT where that fdgs_deform_bwd left it: by the
// same plan_bwd_lists, so the two cannot disagree about which list D2 walked.
static int time_grad_blocks(const fdgs_deform_params* p) { return (int)((npad_of(p->N) + 256 + TG_ROWS - 1) / TG_ROWS); }   // (row lists are padded by < 256 entries)
static int validate_time_grad(const fdgs_deform_params* p, const fdgs_deform_grads* g) {
    int rc = validate_deform(p);
    if (rc) return rc;
    FDGS_REQUIRE(g && g->scratch, "grads/scratch is NULL");
    return FDGS_OK;
}
// the scratch of the fdgs_deform_bwd that ran on (p, g), as the kernels here read it
static void time_grad_sources(const fdgs_deform_params* p, const fdgs_deform_grads* g, const float** DFEAT, const uint32_t** tile_live,
                              const uint32_t** rows, const uint32_t** counters) {
    float* base = reinterpret_cast<float*>(g->scratch);
    const BwdLayout bl = bwd_layout(p);
    const BwdListPlan plan = plan_bwd_lists(p, g);
    *DFEAT = base + bl.DFEAT;
    *tile_live = reinterpret_cast<const uint32_t*>(base + bl.flags);
    *counters = reinterpret_cast<const uint32_t*>(base + bl.counters);
    *rows = plan.by_rows ? reinterpret_cast<const uint32_t*>(base + bl.rows) : nullptr;
}

extern "C" int fdgs_deform_time_grad_scratch_bytes(const fdgs_deform_params* p, size_t* bytes) {
    int rc = validate_deform(p);
    if (rc) return rc;
    FDGS_REQUIRE(bytes, "bytes is NULL");
    *bytes = (size_t)time_grad_blocks(p) * sizeof(float) + 256;
    return FDGS_OK;
}

extern "C" int fdgs_deform_time_grad(void* stream_, const fdgs_deform_params* p, const fdgs_deform_grads* g, void* scratch, float* d_time) {
    int rc = validate_time_grad(p, g);
    if (rc) return rc;
    FDGS_REQUIRE(scratch, "scratch is NULL");
    FDGS_REQUIRE(d_time || (p->time && p->N == 0), "d_time is NULL");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t nout = p->time ? (size_t)p->N : 1;
    if (p->N == 0 || active_heads(p) == 0) {       // (no head active: the deformation is the identity and that backward built no lists)
        if (nout) FDGS_HIP_CHECK(hipMemsetAsync(d_time, 0, nout * sizeof(float), stream));
        return FDGS_OK;
    }
    TimeGradArgs a{};
    a.p = *p; a.sc = aabb_scale(p); a.F = p->C * p->L;
    time_grad_sources(p, g, &a.DFEAT, &a.tile_live, &a.rows, &a.counters);
    a.d_time = p->time ? d_time : nullptr;
    a.partials = reinterpret_cast<float*>(scratch);
    const int blocks = p->time ? cdiv(p->N, TG_ROWS) : time_grad_blocks(p);
    {
        FDGS_TIMED("deform_time_grad_partial", stream);
        if (p->C == 16) hipLaunchKernelGGL(deform_time_grad_partial_kernel<16>, dim3(blocks), dim3(256), 0, stream, a);
        else hipLaunchKernelGGL(deform_time_grad_partial_kernel<32>, dim3(blocks), dim3(256), 0, stream, a);
    }
    FDGS_LAUNCH_CHECK("deform_time_grad_partial", 0, stream);
    if (!p->time) {
        { FDGS_TIMED("deform_time_grad_final", stream); hipLaunchKernelGGL(deform_time_grad_final_kernel, dim3(1), dim3(256), 0, stream, a.partials, blocks, d_time); }
        FDGS_LAUNCH_CHECK("deform_time_grad_final", 0, stream);
    }
    return FDGS_OK;
}

extern "C" int fdgs_deform_time_grad_dfeat(void* stream_, const fdgs_deform_params* p, const fdgs_deform_grads* g, float* dfeat, uint8_t* live) {
    int rc = validate_time_grad(p, g);
    if (rc) return rc;
    if (p->N == 0) return FDGS_OK;
    FDGS_REQUIRE(dfeat && live, "NULL pointer");
    hipStream_t stream = (hipStream_t)stream_;
    TimeGradProbeArgs a{};
    a.N = p->N; a.F = p->C * p->L; a.dfeat = dfeat; a.live = live;
    FDGS_HIP_CHECK(hipMemsetAsync(dfeat, 0, (size_t)p->N * a.F * sizeof(float), stream));
    FDGS_HIP_CHECK(hipMemsetAsync(live, 0, (size_t)p->N, stream));
    if (active_heads(p) == 0) return FDGS_OK;
    time_grad_sources(p, g, &a.DFEAT, &a.tile_live, &a.rows, &a.counters);
    const long long threads = (long long)time_grad_blocks(p) * TG_ROWS * (a.F / 4);
    hipLaunchKernelGGL(deform_time_grad_dfeat_kernel, dim3((unsigned)cdiv(threads, 256)), dim3(256), 0, stream, a);
    FDGS_LAUNCH_CHECK("deform_time_grad_dfeat", 0, stream);
    return FDGS_OK;
}

extern "C" int fdgs_deform_time_grad_host(const fdgs_deform_params* p, const float* dfeat, const uint8_t* live, double* d_time_rows,
                                          double* d_time_sum, double* abs_rows, double* abs_sum) {
    // (only N, C, L, res, planes, aabb, xyz and time / time_scalar are read: everything else of p may be NULL / zero)
    int rc = validate_cells(p, p ? p->xyz : nullptr, dfeat, live, dfeat);
    if (rc) return rc;
    FDGS_REQUIRE(p->C == 16 || p->C == 32, "output_coordinate_dim must be 16 or 32");
    for (int l = 0; l < p->L; l++)
        for (int k = 0; k < 6; k++) FDGS_REQUIRE(p->planes[l][k] != nullptr, "plane pointer is NULL");
    const AabbScale sc = aabb_scale(p);
    const size_t F = (size_t)p->C * p->L;
    double tot = 0.0, tot_abs = 0.0;
    for (size_t n = 0; n < (size_t)p->N; n++) {
        double s = 0.0, sa = 0.0;
        if (live[n]) time_grad_row_host(*p, sc.inv2, n, dfeat + n * F, &s, &sa);       // (a dead row's dfeat is never read)
        if (d_time_rows) d_time_rows[n] = s;
        if (abs_rows) abs_rows[n] = sa;
        tot += s; tot_abs += sa;
    }
    if (d_time_sum) *d_time_sum = tot;
    if (abs_sum) *abs_sum = tot_abs;
    return FDGS_OK;
}

extern "C" int fdgs_hexplane_cells(void* stream_,const fdgs_deform_params* p, int32_t* cells, float* w1, float* dscale, float* q) {
    int rc = validate_cells(p, cells, w1, dscale, q);
    if (rc) return rc;
    if (p->N == 0) return FDGS_OK;
    hipStream_t stream = (hipStream_t)stream_;
    CellsArgs a{};
    a.p = *p; a.sc = aabb_scale(p); a.cells = cells; a.w1 = w1; a.dscale = dscale; a.q = q;
    hipLaunchKernelGGL(hexplane_cells_kernel, dim3(cdiv(p->N, 256)), dim3(256), 0, stream, a);
    FDGS_LAUNCH_CHECK("hexplane_cells_kernel", false, stream);
    return FDGS_OK;
}

extern "C" int fdgs_hexplane_cells_host(const fdgs_deform_params* p, int32_t* cells, float* w1, float* dscale, float* q) {
    int rc = validate_cells(p, cells, w1, dscale, q);
    if (rc) return rc;
    const AabbScale sc = aabb_scale(p);
    const size_t per = (size_t)p->L * 4;
    for (size_t n = 0; n < (size_t)p->N; n++) hexplane_cells_row(*p, sc.inv2, n, cells + n * per * 2, w1 + n * per, dscale + n * per, q + n * 4);
    return FDGS_OK;
}
