/*
 * fdgs.h -- C-ABI of the MI355X-native 4D-Gaussian render path (libfdgs.so, built by hipcc for gfx950).
 *
 * Drop-in boundary.  The reference binds its rasterizer through the pybind module
 * `diff_gaussian_rasterization._C` of the un-vendored submodule named at .gitmodules:5-7 of the reference
 * (call sites gaussian_renderer/__init__.py:14,38-58,120-128; merge_many_4dgs.py:33,85-135;
 * scene/dataset_readers.py:485-508), and its deformation step through the PyTorch modules
 * scene/deformation.py:161-216 + scene/hexplane.py:109-183.  The entry points below are what a binding of this
 * path needs instead: plain pointers and sizes, an explicit hipStream_t (passed as void*), every buffer owned and
 * allocated by the caller, no torch types, no exceptions across the ABI.
 *
 * Conventions
 *   - every function returns 0 on success, a negative FDGS_E_* code otherwise; fdgs_last_error() returns a
 *     thread-local message for the last failure on the calling thread;
 *   - all device pointers are float32 unless stated; "opt" pointers may be NULL;
 *   - matrices are the reference's transposed 4x4s (scene/cameras.py:59-63): flat index m[4*col+row];
 *   - no function synchronises the device except fdgs_bin_prepare (the single num_rendered read-back that the
 *     reference's rasterizer also performs) and the *_debug_sync helpers;
 *   - functions are re-entrant per stream; one host thread per stream.
 */
#ifndef FDGS_H
#define FDGS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FDGS_OK 0
#define FDGS_E_INVALID (-1) /* bad argument / unsupported configuration */
#define FDGS_E_HIP (-2)     /* a HIP runtime call or kernel launch failed */
#define FDGS_E_NOGPU (-3)   /* no gfx950 device visible */

#define FDGS_TILE 16         /* tile edge in pixels (BLOCK_X = BLOCK_Y of the reference rasterizer) */
#define FDGS_SH_COEFFS 16    /* max SH coefficients per channel (degree 3) */

const char* fdgs_last_error(void);
/* ABI version of this header; bump on any signature change. */
int fdgs_abi_version(void);
/* Optional per-kernel timing with HIP events on the launch stream (off by default; used by bench.py for the live
 * roofline measurement).  fdgs_timing_report synchronises the device and writes "kernel_name count total_ms" lines. */
int fdgs_timing_enable(int on);
int fdgs_timing_report(char* buf, size_t buflen, int reset);
/* Development / test knobs (ABI 4; ten since ABI 5, eleven since round 6, thirteen with bin_form and tile_sort_cap, fifteen with bin_count and blend_fwd_form).  The library holds ONE table of integer knobs; it is filled from the environment variables
 * FDGS_<NAME> once, when the library is loaded, and afterwards changes only through fdgs_tuning_set -- no entry point reads the
 * environment.  Knobs select between equivalent kernel forms or launch shapes (same results up to summation order), never semantics:
 *   d1_form (0 | 8 | 16 | 32), d1_wgs, d1_split, skip_dead, d4_mfma, d4_rows_kb, tile_cull (0 = the reference's rectangle lists), rbwd_ppl (-1 = by image size | 4 | 2 | 0),
 *   tile_order (1 = the blending kernels take their tiles heaviest-first, 0 = image order), row_compact (1 = the deformation backward walks
 *   the non-zero rows instead of the non-zero 32-row tiles where it can; 2 = the same with the row lists built by the two-launch form),
 *   d2_form (0 = the weight-stationary backward-data kernel where it applies -- row lists, net_width 128, C*L 32 or 48, five heads or position + scale + rotation --, 32 = the
 *   32-row kernel everywhere),
 *   bin_form (0 = depth sort of the Gaussians + pair expansion + global tile sort, 1 = pairs placed per tile + one LDS sort per tile --
 *   images of up to 16 384 tiles, larger ones keep form 0 --, -1 = by shape; same lists bit for bit), tile_sort_cap (bin_form 1: list
 *   length above which a tile's sort takes the chunk-and-merge path; 0 = the compiled LDS capacity, 4 096; lower values are for tests),
 *   bin_count (bin_form 1, fdgs_raster_fwd_capacity only: 0 = the tiles' pairs are counted by a launch of its own, 1 = by the projection
 *   kernel -- images of up to 5 632 tiles --, with the scan of the counts and the forward's tile order in one launch, 2 = as 1 at every
 *   tile count form 1 runs at; same lists bit for bit; the staged calls always count in fdgs_bin_sort), blend_fwd_form (inner loop of the
 *   blending forward: 0 = one list entry per trip, 1 = two per trip in packed f32; same image, depth and per-pixel state bit for bit).
 * `name` is the lower- or upper-case knob name, with or without the FDGS_ prefix.  Process-global, not thread-safe against running calls:
 * set knobs between frames.  fdgs_tuning_reset restores the load-time values.  See INTEGRATION.md ("Knobs"). */
int fdgs_tuning_set(const char* name, int value);
int fdgs_tuning_get(const char* name, int* value);
int fdgs_tuning_reset(void);
/* Name (gcnArchName) of device `dev` into buf; FDGS_E_NOGPU if none. */
int fdgs_device_arch(int dev, char* buf, size_t buflen);

/* ------------------------------------------------------------------------------------------------------------
 * Rasterizer: replaces _C.rasterize_gaussians / _C.rasterize_gaussians_backward / _C.mark_visible
 * ---------------------------------------------------------------------------------------------------------- */

/* Scratch sizes in bytes. geom: per-Gaussian state (kept for backward); img: per-pixel + per-tile state (kept for
 * backward); binning: sorted (tile, Gaussian) lists for `num_rendered` pairs (kept for backward). */
int fdgs_geom_bytes(int P, size_t* bytes);
int fdgs_img_bytes(int W, int H, size_t* bytes);
int fdgs_binning_bytes(uint32_t num_rendered, int W, int H, size_t* bytes);

typedef struct fdgs_raster_params {
    int P;                  /* number of Gaussians */
    int sh_degree;          /* active degree 0..3 */
    int sh_coeffs;          /* coefficients per channel actually stored per Gaussian (M, <=16) */
    int W, H;               /* image size in pixels */
    float tanfovx, tanfovy;
    float scale_modifier;
    int prefiltered;        /* accepted for API parity; ignored like the reference's non-debug path */
    int debug;              /* nonzero: synchronise + check errors after every kernel */
    const float* bg;        /* [3] device */
    const float* viewmatrix;/* [16] device */
    const float* projmatrix;/* [16] device */
    const float* campos;    /* [3] device */
    const float* means3D;   /* [P,3] */
    const float* shs;       /* opt [P,M,3] (exactly one of shs / colors_precomp) */
    const float* colors_precomp; /* opt [P,3] */
    const float* opacities; /* [P] */
    const float* scales;    /* opt [P,3] (scales+rotations xor cov3D_precomp) */
    const float* rotations; /* opt [P,4] (w,x,y,z), used as given (no normalisation) */
    const float* cov3D_precomp; /* opt [P,6] */
    uint8_t* visibility;    /* opt [P], written by fdgs_preprocess_fwd: 1 where radii > 0 (the `visibility_filter` render() returns,
                               gaussian_renderer/__init__.py:136) -- saves the caller one elementwise launch per frame */
    float* acc_zero;        /* opt [P,16] floats (ABI 5): fdgs_render_fwd zero-fills them on the way.  A training frame passes the buffer it will
                               hand to fdgs_raster_bwd as fdgs_raster_grads::scratch_acc, with scratch_acc_zeroed = 1: the 64 bytes per Gaussian
                               the blending backward accumulates into are then clean without a fill launch between the loss and the backward */
} fdgs_raster_params;

/* Stage 1: per-Gaussian projection (frustum cull, cov3D, EWA cov2D, conic, radius, tile rect, SH->RGB).
 * Writes radii[P] (int32) and fills `geom`. */
int fdgs_preprocess_fwd(void* stream, const fdgs_raster_params* p, void* geom, int32_t* radii);

/* Stage 2: depth-sorts the Gaussians (LSD radix on the fp32 depth bits), scans tiles_touched in depth order and
 * reads the total back to the host: *num_rendered_host = number of (tile, Gaussian) pairs.  This is the one
 * blocking read-back of the path (the reference's rasterizer has the same one). */
int fdgs_bin_prepare(void* stream, const fdgs_raster_params* p, void* geom, uint32_t* num_rendered_host);

/* Stage 3: writes the pairs in depth order, stable-sorts them by tile id (LSD radix), finds per-tile ranges. */
int fdgs_bin_sort(void* stream, const fdgs_raster_params* p, void* geom, void* binning, void* img,
                  uint32_t num_rendered);

/* Stage 4: front-to-back alpha blending per 16x16 tile. out_color [3,H,W], out_depth [1,H,W]. */
/* Capacity mode (ABI 4): stages 1-4 in ONE call and WITHOUT a host synchronisation.  `binning` holds fdgs_binning_bytes(capacity)
 * bytes for a pair count the caller predicts (e.g. 1.5 x the largest count it has seen); the true count stays on the device -- the kernels
 * work on min(true, capacity) pairs -- and reaches *num_rendered_host (pinned host memory) asynchronously (ABI 6: a store of the LAST
 * workgroup of the projection kernel when the word is device-visible -- hipHostGetDevicePointer --, i.e. while the depth sort is still
 * running; a copy node otherwise): pre-set the word to 0xFFFFFFFF and read it once it changed (fdgs_pair_count_wait).  true > capacity
 * means that pairs of this frame were dropped and the image is NOT the reference's -- with binning form 1 (tuning knob bin_form) the
 * frame keeps WHOLE TILES, in image order, while their lists fit: the first tile whose list would end behind `capacity` and every tile
 * after it get the range (0, 0), and no kept list is truncated; with form 0 the FARTHEST pairs are dropped (pairs are emitted in depth
 * order).  Either way nothing is written out of bounds and ranges[:, 1] <= capacity.  The
 * stage-1/2 results in `geom` are complete and valid, so the caller finishes the frame exactly with fdgs_bin_sort + fdgs_render_fwd on a
 * buffer of fdgs_binning_bytes(true) bytes (what the Python host does before it hands the image to anyone: the reference never truncates,
 * SURVEY Appendix B.2).  The buffers are laid out for `capacity`: pass `capacity` as num_rendered to fdgs_raster_bwd /
 * fdgs_binning_field.  P = 0 writes 0 to the word immediately. */
int fdgs_raster_fwd_capacity(void* stream, const fdgs_raster_params* p, void* geom, void* binning, void* img, uint32_t capacity,
                             uint32_t* num_rendered_host, int32_t* radii, float* out_color, float* out_depth);
/* ABI 6: waits (spinning on the pinned word, no hipStreamSynchronize) until the pair count of a frame queued by fdgs_raster_fwd_capacity on
 * `stream` has arrived, and returns it in *value.  The rest of the frame stays queued behind it, so the device does not drain while the
 * host looks at the count.  Error if the stream runs idle without a count (wrong stream / word). */
int fdgs_pair_count_wait(void* stream, const uint32_t* num_rendered_host, uint32_t* value);
int fdgs_render_fwd(void* stream, const fdgs_raster_params* p, const void* geom, const void* binning, void* img,
                    uint32_t num_rendered, float* out_color, float* out_depth);

/* Accumulated opacity (alpha) of a frame, differentiable.  A[y, x] = 1 - T_final = sum_i alpha_i T_i over the entries the pixel blended:
 * what the blend leaves of a background of ones, the coverage a mask / silhouette loss, an opacity regulariser, a composite over a background
 * IMAGE (render with bg = 0, then render + (1 - A) * B) or a normalised depth (depth / A) needs.
 *   Forward: fdgs_render_fwd_alpha and fdgs_raster_fwd_capacity_alpha are fdgs_render_fwd and fdgs_raster_fwd_capacity with one more image,
 *   out_alpha [H*W] floats (4-byte aligned): 1.0f - T of the very T the kernel stores per pixel for the backward, one more store where the
 *   pixel's results are written.  A pixel with an empty list gets exactly 0; P = 0 or no pairs: all zeros.  out_alpha = NULL is the old call
 *   (the old entry points are that case of the same implementation).
 *   Backward: fdgs_raster_bwd_alpha is fdgs_raster_bwd with dL_dalpha [H*W] floats (4-byte aligned), the gradient of the loss to A.  Every
 *   blended entry i of a pixel gets dL/dalpha_i += dL_dalpha * T_final / (1 - alpha_i) -- the background term's factor with the sign turned,
 *   so the blending backward forms its per-pixel background term from (bg . dL_dcolor - dL_dalpha) and walks the lists as before: nothing
 *   per list entry is added.  Entries behind the pixel's stop (T (1 - alpha) < 1e-4) get nothing and the 0.99 clamp of alpha is
 *   straight-through, both as for colour.  Everything behind the blending backward -- the conic, mean2D and opacity sums, dL_dmeans2D, the
 *   live-row flags, the deformation epilogue, fdgs_camera_grad on the same scratch_acc -- includes alpha's share by construction.
 *   dL_dalpha = NULL is the old call.  A loss on alpha alone passes a zero dL_dcolor (it stays required). */
int fdgs_render_fwd_alpha(void* stream, const fdgs_raster_params* p, const void* geom, const void* binning, void* img,
                          uint32_t num_rendered, float* out_color, float* out_depth, float* out_alpha);
int fdgs_raster_fwd_capacity_alpha(void* stream, const fdgs_raster_params* p, void* geom, void* binning, void* img, uint32_t capacity,
                                   uint32_t* num_rendered_host, int32_t* radii, float* out_color, float* out_depth, float* out_alpha);

/* Optional epilogue of fdgs_raster_bwd for the fused render() path (deformation -> rasterizer): the per-Gaussian chain rule
 * writes its results straight in the form fdgs_deform_bwd consumes -- the packed pre-activation output-gradient rows G[Npad][64]
 * (columns 0-2 position, 3-5 log-scale, 6-9 raw quaternion, 10 opacity logit, 16-63 SH; activation Jacobians of
 * gaussian_renderer/__init__.py:97-99 applied when `activate`) and the identity paths of `out = in + delta` accumulated into the
 * parameter gradients -- instead of dL_dmeans3D / dL_dscales / dL_drotations / dL_dopacity / dL_dsh, which are then not written.
 * G is the START of the scratch buffer later handed to fdgs_deform_bwd (fdgs_deform_grads::scratch) with packed_rows_ready = 1 / 2 / 3
 * for tile_flags = 0 / 1 / 2.
 * Saves one kernel and a write + read of 236 bytes per Gaussian between the two backward stages. */
typedef struct fdgs_raster_deform_epilogue {
    int activate;                /* the scales / rotations / opacities the rasterizer received are exp / normalize / sigmoid outputs */
    int Npad;                    /* rows of G: fdgs_deform_bwd's padded Gaussian count (multiple of 128, >= P) */
    const float* rot_norm;       /* [P] norm of the raw quaternion (activate = 1), fdgs_deform_out::rot_norm */
    float* G;                    /* [Npad,64], every row written (rows >= P zero) unless tile_flags = 2 */
    float* d_xyz; float* d_scales; float* d_rotations; float* d_opacity;   /* identity paths (any may be NULL) */
    float* d_shs_dc; float* d_shs_rest;                                    /* strides in floats as in fdgs_deform_params */
    int shs_dc_stride; int shs_rest_stride;
    int assign;                  /* 0: the identity paths are accumulated (+=, caller zero-fills); 1: they are ASSIGNED (=): the caller
                                    needs no zero fill of these six arrays -- fdgs_deform_bwd, which runs afterwards, only ever adds to
                                    d_xyz (the HexPlane coordinate gradient) */
    int tile_flags;              /* 1: G is followed by uint32 tile_live[Npad/32] (i.e. at (uint32_t*)(G + Npad*64)), written here:
                                    bit r of tile_live[t] is set when packed row 32t + r has a non-zero entry (a tile is live when its word is
                                    non-zero; ABI 5: the word is the row mask, it used to be 0 / 1).  Culled, occluded and
                                    off-screen Gaussians get all-zero rows (the reference gives them no gradient either,
                                    gaussian_renderer/__init__.py:134-138); fdgs_deform_bwd (packed_rows_ready = 2) then skips whole tiles of
                                    them -- exact, a zero row adds exactly zero to every sum -- and, with saved activations on spatially ordered
                                    input, walks only the non-zero ROWS (tuning knob row_compact).
                                    2: as 1, and the 32 rows of a tile flagged 0 are NOT written (their content is unspecified): the caller
                                    MUST hand G to fdgs_deform_bwd with packed_rows_ready = 3, which never reads them (the one dead tile it
                                    may use as padding is zero-filled there).
                                    0: no flags (packed_rows_ready = 1: fdgs_deform_bwd walks every tile) */
    float* zero_fill;            /* opt: a float range this kernel zero-fills on the way (16-byte aligned; zero_floats a multiple of 4): the part
                                    of the caller's gradient arena that fdgs_deform_bwd ACCUMULATES into (planes, MLP) -- saves a fill launch */
    size_t zero_floats;
} fdgs_raster_deform_epilogue;

typedef struct fdgs_raster_grads {
    const float* dL_dcolor;  /* [3,H,W] */
    const float* dL_ddepth;  /* opt [1,H,W] */
    /* outputs: every row is written by fdgs_raster_bwd (zeros for culled Gaussians); no caller-side zero fill needed */
    float* dL_dmeans2D;      /* [P,3]: x,y in NDC units, z = 0 (the reference's viewspace_points.grad) */
    float* dL_dmeans3D;      /* [P,3] */
    float* dL_dopacity;      /* [P] */
    float* dL_dcolors;       /* [P,3] gradient of the blended per-Gaussian rgb (== dL/dcolors_precomp) */
    float* dL_dsh;           /* opt [P,M,3] (required when shs was given) */
    float* dL_dscales;       /* opt [P,3] */
    float* dL_drotations;    /* opt [P,4] */
    float* dL_dcov3D;        /* [P,6] */
    /* scratch owned by the caller: [P,16] floats (one 64-byte gradient line per Gaussian, see render.hip) */
    float* scratch_acc;
    /* opt: see above (requires shs + scales/rotations inputs, 16 SH coefficients) */
    const fdgs_raster_deform_epilogue* deform_epilogue;
    int scratch_acc_zeroed;  /* 1: scratch_acc is the buffer the forward of THIS state zero-filled (fdgs_raster_params::acc_zero) and no backward
                                has used it since; 0: fdgs_raster_bwd fills it */
} fdgs_raster_grads;

/* Backward of stages 4 and 1 (back-to-front blending gradients, then per-Gaussian chain rule). */
int fdgs_raster_bwd(void* stream, const fdgs_raster_params* p, const void* geom, const void* binning,
                    const void* img, uint32_t num_rendered, const fdgs_raster_grads* g);
/* ... with the gradient of the accumulated opacity (see fdgs_render_fwd_alpha above); dL_dalpha opt [H*W] */
int fdgs_raster_bwd_alpha(void* stream, const fdgs_raster_params* p, const void* geom, const void* binning,
                          const void* img, uint32_t num_rendered, const fdgs_raster_grads* g, const float* dL_dalpha);

/* Antialiased splatting: opacity compensation for the dilation (the EWA normalisation of Mip-Splatting; the upstream rasterizer's
 * `antialiasing`, gsplat's rasterize_mode = "antialiased").  The projection adds 0.3 to the diagonal of every projected covariance, which
 * widens a splat without lowering its peak: a splat far below a pixel blends much more than it carries.  With A, b, C the projected
 * covariance before the dilation, a = A + 0.3, c = C + 0.3:
 *       D0 = A C - b^2    D1 = a c - b^2    r = D0 / D1    h = sqrt(max(2.5e-5, r))        (the floor is upstream's)
 * and the opacity the frame blends with is opacity * h.  It is what the projection kernel writes into recB.y (fdgs_geom_field 2) and what
 * the exact tile culling sets its ellipse up from.  Nothing else changes: conic, radius, rect, depth, colour and every cull decision of the
 * projection use the dilated covariance as before, so radii, visibility and densification statistics are those of the plain frame (only the
 * pair count can fall: h <= 1 tightens the cull ellipse).
 *   Forward: fdgs_preprocess_fwd_aa is fdgs_preprocess_fwd, fdgs_raster_fwd_capacity_aa is fdgs_raster_fwd_capacity_alpha (out_alpha opt),
 *   with the compensation.  fdgs_bin_prepare, fdgs_bin_sort, fdgs_render_fwd(_alpha) and every replay pass (fdgs_render_pick,
 *   fdgs_render_contrib, fdgs_render_features and its backward, the motion blend) are unchanged: they read recB and the cull mask the
 *   projection wrote and nothing of the opacity input, so they follow an antialiased geom as it stands.
 *   Backward: fdgs_raster_bwd_aa is fdgs_raster_bwd_alpha (dL_dalpha opt).  The blending backward is the same; its opacity sum is then
 *   g = dL/d(opacity * h).  The per-Gaussian chain rule returns dL_dopacity = h * g (the epilogue: before the sigmoid's Jacobian) and, for r
 *   above the floor, adds dL/dr = g * opacity / (2 h) through
 *       dr/da = (C D1 - D0 c) / D1^2    dr/dc = (A D1 - D0 a) / D1^2    dr/db = 2 b (D0 - D1) / D1^2
 *   to the covariance's gradient, from where it reaches dL_dcov3D, scales, rotations and the means like the conic's share (same clamp
 *   conventions).  At or below the floor that path is exactly zero.  It reads p->opacities: the opacities the forward received.
 *   fdgs_camera_grad_aa is fdgs_camera_grad of such a state (the compensation's share of the view matrix' gradient included).
 *   A backward or camera-gradient call MUST take the case of the forward of its state: the state does not record it.
 *   Host twins, as fdgs_preprocess_host / fdgs_preprocess_bwd_host / fdgs_camera_grad_host: fdgs_preprocess_host_aa also returns
 *   opacity_eff[P] = opacity * h (0 for a culled Gaussian; it reads p->opacities), fdgs_preprocess_bwd_host_aa also takes d_opacity[P] (= g)
 *   and returns dL_dopacity[P], fdgs_camera_grad_host_aa also takes d_opacity[P].
 * The old entry points are the other case of the same implementation (a template switch on the kernels: they keep their instructions). */
int fdgs_preprocess_fwd_aa(void* stream, const fdgs_raster_params* p, void* geom, int32_t* radii);
int fdgs_raster_fwd_capacity_aa(void* stream, const fdgs_raster_params* p, void* geom, void* binning, void* img, uint32_t capacity,
                                uint32_t* num_rendered_host, int32_t* radii, float* out_color, float* out_depth, float* out_alpha);
int fdgs_raster_bwd_aa(void* stream, const fdgs_raster_params* p, const void* geom, const void* binning,
                       const void* img, uint32_t num_rendered, const fdgs_raster_grads* g, const float* dL_dalpha);
int fdgs_camera_grad_aa(void* stream, const fdgs_raster_params* p, const void* geom, const float* scratch_acc, void* scratch,
                        float* out /* 48 floats, 16-byte aligned */);
int fdgs_preprocess_host_aa(const fdgs_raster_params* p, int32_t* radii, float* xy, float* conic, float* depth, float* rgb,
                            uint32_t* clamped, float* cov3D, uint32_t* rect, uint32_t* tiles, float* opacity_eff);
int fdgs_preprocess_bwd_host_aa(const fdgs_raster_params* p, const uint32_t* tiles, const uint32_t* clamped, const float* cov3D,
                                const float* d_xy, const float* d_conic, const float* d_rgb, const float* d_depth, const float* d_opacity,
                                float* dL_dmeans2D, float* dL_dmeans3D, float* dL_dsh, float* dL_dscales, float* dL_drotations,
                                float* dL_dcov3D, float* dL_dopacity);
int fdgs_camera_grad_host_aa(const fdgs_raster_params* p, const uint32_t* tiles, const uint32_t* clamped, const float* cov3D,
                             const float* d_xy, const float* d_conic, const float* d_rgb, const float* d_depth, const float* d_opacity,
                             double* out /* 48 */);

/* Absolute screen-space gradients (the "absgrad" of AbsGS, gsplat's means2d.absgrad): the densification statistic that does not cancel.
 * dL_dmeans2D is the SIGNED sum over the pixels that blended a Gaussian; for a Gaussian that is too large the pixels on either side of its
 * centre pull in opposite directions and the sum cancels, so the splats that most need splitting never reach the threshold.  For Gaussian i,
 * with the loss gradient reaching the frame through colour, depth and (where given) alpha:
 *       abs_i = ( sum_p |dL_p/dx_i| W/2 ,  sum_p |dL_p/dy_i| H/2 ,  0 )
 * p runs over the pixels that blended i -- the `valid` decisions of the signed sum: inside n_contrib, power <= 0, alpha >= 1/255 --, and
 * dL_p/d(x, y) is that pixel's WHOLE contribution to slots 0 and 1 of the accumulator line: summed over the three image gradients first,
 * then taken absolute.  The scaling to NDC units is the one of dL_dmeans2D (a positive factor: it commutes with the absolute value).  Rows
 * that are culled or that no pixel blended are exactly +0, the third column is exactly 0.  On an antialiased frame the per-pixel gradient is
 * the one that frame's blending backward forms; nothing else is needed.
 *   fdgs_raster_bwd_abs is fdgs_raster_bwd_alpha (antialiased = 0) or fdgs_raster_bwd_aa (antialiased != 0) of the same arguments, which
 *   also writes dL_dmeans2D_abs [P,3] floats (4-byte aligned), every row.  The blending backward adds the two absolute sums into slots 10
 *   and 11 of the Gaussian's scratch_acc line (same reductions, same atomic line-op; slots 12..15 stay zero), the per-Gaussian chain rule
 *   writes them out, with the deformation epilogue as without.  Every other output is what the sibling call writes.
 *   dL_dmeans2D_abs = NULL IS the sibling call: the same implementation, the kernels of a frame that does not ask (slots 10..15 stay zero).
 *   P = 0: nothing is written.  No pairs: zeros. */
int fdgs_raster_bwd_abs(void* stream, const fdgs_raster_params* p, const void* geom, const void* binning, const void* img,
                        uint32_t num_rendered, const fdgs_raster_grads* g, const float* dL_dalpha /* opt */,
                        int antialiased, float* dL_dmeans2D_abs /* [P,3], 4-byte aligned */);

/* Frustum test only (replaces _C.mark_visible): present[P] (uint8) = 1 where p_view.z > 0.2. */
int fdgs_mark_visible(void* stream, int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                      uint8_t* present);

/* Host twins of the two per-Gaussian projection kernels (stage 1 and the chain-rule half of fdgs_raster_bwd): a loop over the Gaussians on
 * the CPU around the very functions of csrc/gs_math.h the kernels call, so the projection arithmetic can be checked without a GPU.  Every
 * pointer -- those inside `p` included -- is a HOST pointer.  `p` is validated as for fdgs_preprocess_fwd, so bg must be non-NULL (and campos
 * with SH inputs) although the values of bg, opacities, visibility and acc_zero are never read.  Not bit for bit the
 * device's result: the kernels may contract a * b + c, the host build does not.
 *   fdgs_preprocess_host: per Gaussian radii[P], xy[P,2] (pixels), conic[P,3] (xx, xy, yy), depth[P], rgb[P,3], clamped[P] (bit c = channel c
 *     was clamped at 0), cov3D[P,6], rect[P,2] (xmin|ymin<<16, xmax|ymax<<16) and tiles[P] = tiles of the 3-sigma square (what the kernel
 *     counts without exact tile culling).  A culled Gaussian gets zeros everywhere.
 *   fdgs_preprocess_bwd_host: tiles / clamped / cov3D as the forward twin left them; the per-Gaussian sums the blending backward leaves in
 *     fdgs_raster_grads::scratch_acc as separate arrays: d_xy[P,2] = dL/d(xy) in pixel units, d_conic[P,3] = dL/d(conic) with the kernel's
 *     half-weight xy entry, d_rgb[P,3], d_depth[P] (NULL: zeros).  Outputs as fdgs_raster_grads: dL_dmeans2D[P,3] (NDC units, z = 0),
 *     dL_dmeans3D[P,3], dL_dsh[P,M,3] (with shs), dL_dscales[P,3] / dL_drotations[P,4] (with scales and rotations), dL_dcov3D[P,6].  A
 *     Gaussian without tiles gets zero rows, as from the kernel. */
int fdgs_preprocess_host(const fdgs_raster_params* p, int32_t* radii, float* xy, float* conic, float* depth, float* rgb,
                         uint32_t* clamped, float* cov3D, uint32_t* rect, uint32_t* tiles);
int fdgs_preprocess_bwd_host(const fdgs_raster_params* p, const uint32_t* tiles, const uint32_t* clamped, const float* cov3D,
                             const float* d_xy, const float* d_conic, const float* d_rgb, const float* d_depth,
                             float* dL_dmeans2D, float* dL_dmeans3D, float* dL_dsh, float* dL_dscales, float* dL_drotations,
                             float* dL_dcov3D);

/* The camera's gradient: dL/d(viewmatrix, projmatrix, campos) of the frame whose fdgs_raster_bwd has just run -- the three tensors every
 * other call reads as constants.  Each visible Gaussian's share comes from the sums its chain rule already takes (csrc/gs_math.h
 * camera_terms); these calls add the shares up.  Row-vector convention, row-major matrices, entry [4*r + c].
 *   out[48], ASSIGNED (not accumulated):  [0,16) dL/dviewmatrix (column 3 exactly 0)   [16,32) dL/dprojmatrix (column 2 exactly 0)
 *                                         [32,35) dL/dcampos (0 with colors_precomp)    [35,48) zeros
 *   fdgs_camera_grad_scratch_bytes: size of `scratch` for P Gaussians (one 128-byte row of partial sums per 256 Gaussians).
 *   fdgs_camera_grad: call it after fdgs_raster_bwd of the same state (same p, same geom) with the scratch_acc that call used --
 *     fdgs_raster_bwd only reads the accumulator once the blending backward has filled it, so it is intact.  Reads tiles, clamped and cov3D
 *     from geom.  Two launches (per-workgroup partial rows, then one workgroup adds the rows in a fixed order) and no float atomics: for a
 *     given scratch_acc the 48 floats are the same bits every run.  scratch_acc, scratch and out are device pointers, 16-byte aligned.
 *     P == 0 writes zeros (geom, scratch_acc and scratch may then be NULL).
 *   fdgs_camera_grad_host: the host twin -- the loop of fdgs_preprocess_bwd_host, with that call's inputs (host pointers, d_depth NULL:
 *     zeros), around the same function, summed in double.  A difference to the device is the device's float summation and contraction. */
int fdgs_camera_grad_scratch_bytes(int P, size_t* bytes);
int fdgs_camera_grad(void* stream, const fdgs_raster_params* p, const void* geom, const float* scratch_acc, void* scratch,
                     float* out /* 48 floats, 16-byte aligned */);
int fdgs_camera_grad_host(const fdgs_raster_params* p, const uint32_t* tiles, const uint32_t* clamped, const float* cov3D,
                          const float* d_xy, const float* d_conic, const float* d_rgb, const float* d_depth, double* out /* 48 */);

/* Test/diagnostic access to geom fields (device pointers into `geom`):
 * 0 depth f32[P]; 1 recA float4[P] (x,y,conic.xx,conic.xy); 2 recB float4[P] (conic.yy,opacity,depth,0);
 * 3 recC float4[P] (r,g,b,0); 4 cov3D f32[P,6]; 5 tiles_touched u32[P]; 6 clamped u32[P] (bit c = channel c);
 * 7 rect u32[P,2] (xmin|ymin<<16, xmax|ymax<<16); 8 sorted Gaussian ids u32[P]; 9 point_offsets u32[P] (inclusive, depth
 * order; ABI 5: LOCAL to chunks of 4096 Gaussians -- the pair expansion adds the totals of the chunks in front itself).
 * Fields 8 and 9 are defined only for binning form 0 (tuning knob bin_form): form 1 has no depth sort of the Gaussians and does not
 * produce them (field 8 then holds the identity the projection kernel wrote, field 9 is not written).
 *
 * Field 3 (recC) may be REWRITTEN between two fdgs_render_fwd calls of a FORWARD-ONLY frame: a frame queued with acc_zero == NULL that
 * no fdgs_raster_bwd will follow.  recC is the only thing the blend reads that depends on colour, the blend is linear in it and never
 * clamps it, so a second fdgs_render_fwd blends whatever three per-Gaussian values now stand there over the very same sorted lists
 * (what the motion pass does: fdgs_motion_rows writes straight into recC).  The second call must get the same geom, binning and img and
 * the num_rendered the buffers were laid out for; it gets its own out_color and a background of zeros (a copy of the params whose bg
 * points at three device zeros and whose acc_zero is NULL).  It leaves final_T, n_contrib, the ranges and the tile order as they were --
 * those decisions do not depend on colour -- and writes to out_depth the depth the first call wrote.  A second fdgs_render_fwd does not
 * touch an alpha image the first call wrote (fdgs_render_fwd_alpha); a second fdgs_render_fwd_alpha writes the same alpha again. */
int fdgs_geom_field(void* geom, int P, int which, void** ptr);
/* 0 sorted pair Gaussian ids u32[R]; 1 sorted pair tile ids u32[R]. */
int fdgs_binning_field(void* binning, uint32_t num_rendered, int W, int H, int which, void** ptr);
/* 0 final_T f32[H*W]; 1 n_contrib u32[H*W]; 2 ranges u32[ntiles,2]; 3 per-tile walk length of the backward u32[ntiles] (max n_contrib);
 * 4 / 5 heaviest-first tile order of the forward / backward, u32[8][per_xcd] with per_xcd = ceil(ceil(gy / 2) / 8) * 2 * gx (0xFFFFFFFF =
 * padding slot; written only while the tuning knob tile_order is on and per_xcd <= 8192). */
int fdgs_img_field(void* img, int W, int H, int which, void** ptr);

/* ------------------------------------------------------------------------------------------------------------
 * Deformation field: replaces deform_network.forward (scene/deformation.py:185-212) + the activations of
 * gaussian_renderer/__init__.py:97-99 when `activate` is set.
 * ---------------------------------------------------------------------------------------------------------- */

#define FDGS_MAX_LEVELS 4
#define FDGS_HEAD_POS 0
#define FDGS_HEAD_SCALE 1
#define FDGS_HEAD_ROT 2
#define FDGS_HEAD_OPACITY 3
#define FDGS_HEAD_SHS 4
#define FDGS_NUM_HEADS 5

typedef struct fdgs_deform_params {
    int N;                 /* Gaussians */
    int C;                 /* features per plane (output_coordinate_dim: 16 or 32) */
    int L;                 /* levels (len(multires) <= 4) */
    int W;                 /* net_width (64 or 128) */
    int head_on[FDGS_NUM_HEADS]; /* 1 = head active (not no_dx / no_ds / no_dr / no_do / no_dshs) */
    int activate;          /* 1: outputs are exp(scale), normalize(rot), sigmoid(opacity) */
    int res[FDGS_MAX_LEVELS][4]; /* per level: resolution of axes x,y,z,t */
    /* planes: channel-LAST device arrays [res_j][res_i][C] for pair k=(i,j) in order (0,1),(0,2),(0,3),(1,2),(1,3),(2,3) */
    const float* planes[FDGS_MAX_LEVELS][6];
    float aabb[6];         /* aabb[0..2] = "max" row, aabb[3..5] = "min" row of the reference's HexPlaneField.aabb */
    const float* w0; const float* b0;               /* feature_out.0: [W, C*L], [W] */
    const float* w1[FDGS_NUM_HEADS]; const float* b1[FDGS_NUM_HEADS]; /* <head>.1: [W,W],[W] */
    const float* w2[FDGS_NUM_HEADS]; const float* b2[FDGS_NUM_HEADS]; /* <head>.3: [k,W],[k], k = 3,3,4,1,48 */
    /* per-Gaussian inputs */
    const float* xyz;      /* [N,3] */
    const float* scales;   /* [N,3] log-scales */
    const float* rotations;/* [N,4] */
    const float* opacity;  /* [N,1] logits */
    const float* shs_dc;   /* features_dc:   3 floats per Gaussian at shs_dc[n*shs_dc_stride + m] */
    const float* shs_rest; /* features_rest: 45 floats per Gaussian at shs_rest[n*shs_rest_stride + m] */
    int shs_dc_stride;     /* 3 for a separate [N,1,3] tensor; 48 when both point into one [N,16,3] tensor */
    int shs_rest_stride;   /* 45 for a separate [N,15,3] tensor; 48 (with shs_rest = shs + 3) for a combined one */
    const float* time;     /* [N] per-Gaussian time, or NULL to use time_scalar for every Gaussian */
    float time_scalar;
} fdgs_deform_params;

typedef struct fdgs_deform_out {
    float* xyz;       /* [N,3] */
    float* scales;    /* [N,3] */
    float* rotations; /* [N,4] */
    float* opacity;   /* [N,1] */
    float* shs;       /* [N,16,3] */
    float* rot_norm;  /* opt [N]: |r + dr| before normalisation (written when activate=1; the backward needs it) */
    void* saved;      /* opt, fdgs_deform_saved_bytes() bytes: when given, the forward also stores the HexPlane features,
                         relu(hidden) and relu(h1) of every active head; handing the same buffer to fdgs_deform_bwd lets the
                         backward skip the gather and the recomputation of those layers (about 40 % of its MFMA work) */
    void* packed;     /* opt, fdgs_deform_pack_bytes() bytes of scratch: when given (and C % 16 == 0), the forward first re-orders W0 and the
                         heads' W1 into it as the operand streams of its matrix-core loops (contiguous 1-KB loads instead of 64 cache lines
                         per request) and runs its 16-Gaussians-per-wave form, two waves per SIMD -- the faster form inside a frame
                          and what the Python host hands over by default; NULL: the 32-Gaussian form on the row-major
                         weights.  Same results up to summation order, same `saved` format.  (Tuning knob d1_form = 32 forces the
                         32-Gaussian form for A/B runs.) */
} fdgs_deform_out;

int fdgs_deform_saved_bytes(const fdgs_deform_params* p, size_t* bytes);
int fdgs_deform_pack_bytes(const fdgs_deform_params* p, size_t* bytes);
int fdgs_deform_fwd(void* stream, const fdgs_deform_params* p, const fdgs_deform_out* out);

typedef struct fdgs_deform_grads {
    /* incoming gradients w.r.t. the outputs of fdgs_deform_fwd (same `activate` setting); any may be NULL (=0) */
    const float* g_xyz; const float* g_scales; const float* g_rotations; const float* g_opacity; const float* g_shs;
    /* forward outputs (needed when activate=1 for the activation Jacobians) */
    const float* out_scales; const float* out_rotations; const float* out_opacity; const float* rot_norm;
    /* outgoing gradients; ACCUMULATED into (+=): the caller zero-fills.  Any may be NULL (skipped). */
    float* d_xyz; float* d_scales; float* d_rotations; float* d_opacity;
    float* d_shs_dc; float* d_shs_rest; /* laid out with the strides of the inputs (shs_dc_stride / shs_rest_stride) */
    float* d_planes[FDGS_MAX_LEVELS][6]; /* channel-last like `planes` */
    float* d_w0; float* d_b0;
    float* d_w1[FDGS_NUM_HEADS]; float* d_b1[FDGS_NUM_HEADS];
    float* d_w2[FDGS_NUM_HEADS]; float* d_b2[FDGS_NUM_HEADS];
    /* scratch owned by the caller, fdgs_deform_bwd_scratch_bytes() bytes */
    void* scratch;
    /* opt: the `saved` buffer the forward of the SAME parameters / inputs filled (NULL: everything is recomputed) */
    const void* saved;
    /* 0: fdgs_deform_bwd packs the rows (and computes the per-tile flags) itself.
     * 1: `scratch` already starts with the packed gradient rows and the identity paths were applied (fdgs_raster_bwd's epilogue,
     *    tile_flags = 0); the g_* / out_* / rot_norm pointers above are then ignored.  No flags: every tile is walked.
     * 2: as 1, and the rows are followed by the per-tile non-zero flags (epilogue tile_flags = 1): all-zero tiles are skipped.
     * 3: as 2, and the rows of tiles flagged 0 were NOT written (epilogue tile_flags = 2): all-zero tiles are ALWAYS skipped.
     * (The tuning knob skip_dead = 0 makes modes 0 and 2 walk every tile for A/B runs; it cannot affect modes 1 and 3.) */
    int packed_rows_ready;
    /* hint, never needed for correctness: 1 = consecutive Gaussians are spatial neighbours (the set is kept along a space-filling
     * curve, fdgs.densify.spatial_reorder): with one frame time for all Gaussians the plane gradient then runs as the windowed
     * matrix-core splat (one atomic line per touched texel of a chunk's window); 0 = unknown order: per-corner atomics, which are
     * faster on unordered input (0.41 vs 0.72 ms at 300 k) and slower on ordered input (0.69 vs 0.31 ms) */
    int spatially_ordered;
} fdgs_deform_grads;

int fdgs_deform_bwd_scratch_bytes(const fdgs_deform_params* p, size_t* bytes);
int fdgs_deform_bwd(void* stream, const fdgs_deform_params* p, const fdgs_deform_grads* g);
/* Diagnostics (bench.py's FLOP accounting): after fdgs_deform_bwd on `scratch`, out_host[0] = 32-row tiles the backward processed
 * (tiles with a non-zero packed gradient row, + at most 3 of padding; in the row-list form -- tuning knob row_compact, saved activations,
 * spatially ordered input -- the 32-row units of the list of non-zero ROWS, padded to whole chunks), out_host[1] = tiles in total (Npad / 32),
 * out_host[2] = plane-gradient chunks processed, out_host[3] = chunks in total.  Synchronises the stream. */
int fdgs_deform_bwd_live_tiles(void* stream, const fdgs_deform_params* p, const void* scratch, uint32_t* out_host);

/* HexPlane index arithmetic (additions to ABI 6; no existing signature changed): a probe of the texel cells every deformation kernel takes,
 * and its host twin.  The arithmetic is one host/device function per operation (csrc/hexplane_ops.h, contraction off): q = ((x - aabb[i]) *
 * (2 / (aabb[3+i] - aabb[i]))) - 1, three roundings like the reference's normalize_aabb; pixel = ((q + 1) * 0.5) * (size - 1), border clamp,
 * floor.  The *_host twin returns, over host arrays and without a GPU, bit for bit what the device entry point writes, and both equal
 * F.grid_sample(align_corners=True, padding_mode='border') on float32 (tests/golden/hexplane_cells.npz).
 *   p       only N, xyz, time / time_scalar, aabb, L and res are read; planes (and everything else) may be NULL / zero
 *   cells   int32 [N][L][4][2]: (i0, i1) of axes x, y, z, t per level, i1 = min(i0 + 1, size - 1)
 *   w1      float [N][L][4]: weight of i1 (the weight of i0 is 1 - w1)
 *   dscale  float [N][L][4]: d pixel / d coordinate = (size - 1) / 2, 0 where the border clamp is active
 *   q       float [N][4]: the normalised coordinates (q[3] = the time, which is never normalised)
 * The probe is ONE launch on `stream` of a one-thread-per-Gaussian kernel; it is never part of a frame. */
int fdgs_hexplane_cells(void* stream, const fdgs_deform_params* p, int32_t* cells, float* w1, float* dscale, float* q);
int fdgs_hexplane_cells_host(const fdgs_deform_params* p, int32_t* cells, float* w1, float* dscale, float* q);

/* The gradient of the time (additions to ABI 6; no existing signature or struct changed).  The time reaches the deformation only through the
 * fourth HexPlane coordinate, so dL/dt is the coordinate gradient of the three time planes:
 *   dt_n = sum_lvl sum_c dfeat[n][lvl C + c] * sum_{k in (x,t),(y,t),(z,t)} (prod_{k' != k} v_k'[c]) * dscale_t * sum_x w_x (P_k[t1][x][c] - P_k[t0][x][c])
 * with dfeat = dL/d(HexPlane features), which fdgs_deform_bwd forms and leaves in its scratch.  dscale_t = 0 where the border clamp is
 * active: a time at or beyond the last time row has a gradient of exactly 0.  Opt-in: a frame that does not call these runs what it ran.
 *   fdgs_deform_time_grad   is called AFTER fdgs_deform_bwd(stream, p, g), with the same p, g (and the same tuning knobs) on the same stream,
 *       and reads that call's scratch.  d_time is float [N] when p->time is set (the kernel stores every row, 0 for rows without a gradient:
 *       no fill by the caller), float [1] otherwise: the sum over the rows, reduced in a fixed order without float atomics (per workgroup in
 *       float through LDS, the workgroups' partials by one workgroup in double) -- for a given scratch the same bits on every run.
 *       `scratch`: fdgs_deform_time_grad_scratch_bytes(p) bytes.  N == 0, no active head or no row with a gradient give zeros.
 *       Two launches (one with p->time), none of them on the default frame path.
 *   fdgs_deform_time_grad_dfeat   a probe (tests): dfeat of that backward in Gaussian order, float [N][C*L] (0 for dead rows), and one
 *       byte per row, 1 = the backward computed the row's dfeat.
 *   fdgs_deform_time_grad_host   the host twin over host arrays (of p only N, C, L, res, planes, aabb, xyz, time / time_scalar are read): the
 *       same index arithmetic (csrc/hexplane_ops.h), every sum in double.  Rows with live[n] == 0 are not read and give 0.  d_time_rows /
 *       abs_rows double [N], d_time_sum / abs_sum double [1]: the sums of the addends and of their absolute values, per row and over all
 *       rows; any of the four may be NULL. */
int fdgs_deform_time_grad_scratch_bytes(const fdgs_deform_params* p, size_t* bytes);
int fdgs_deform_time_grad(void* stream, const fdgs_deform_params* p, const fdgs_deform_grads* g, void* scratch, float* d_time);
int fdgs_deform_time_grad_dfeat(void* stream, const fdgs_deform_params* p, const fdgs_deform_grads* g, float* dfeat, uint8_t* live);
int fdgs_deform_time_grad_host(const fdgs_deform_params* p, const float* dfeat, const uint8_t* live, double* d_time_rows, double* d_time_sum,
                               double* abs_rows, double* abs_sum);

/* ------------------------------------------------------------------------------------------------------------
 * Loss-side helper for the frame-parallel driver: accumulates [sum|a-b|, sum (a-b)^2, n] into acc[3] (device,
 * caller zero-fills) and optionally writes dL/da = sign(a-b)*scale.  (utils/loss_utils.py:20-21, image_utils.py:17-38)
 * ---------------------------------------------------------------------------------------------------------- */
int fdgs_l1_stats(void* stream, size_t n, const float* a, const float* b, float grad_scale, float* grad_out_opt,
                  float* acc);
/* Same statistics ASSIGNED to acc[3] (no zero fill by the caller, no same-address float atomics, sums added in a fixed order: deterministic).
 * `scratch`: fdgs_l1_stats_scratch_bytes() bytes of device memory, zero-filled ONCE at allocation (it holds a self-resetting ticket counter);
 * one scratch per stream. */
int fdgs_l1_stats_scratch_bytes(size_t* bytes);
int fdgs_l1_stats_assign(void* stream, size_t n, const float* a, const float* b, float grad_scale, float* grad_out_opt,
                         float* acc, void* scratch);

/* ------------------------------------------------------------------------------------------------------------
 * Image losses of the step right after render() (train.py:201-214): l1_loss (utils/loss_utils.py:20-21), the sum of
 * squares psnr() needs (utils/image_utils.py:17-38) and ssim() (utils/loss_utils.py:40-66: 11x11 Gaussian window,
 * sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2), forward value and gradient wrt the rendered image.
 * img / gt: [items][channels][H][W] contiguous f32 (device).
 *   fwd: acc[item][4] += { sum|img-gt|, sum (img-gt)^2, channels*H*W, sum of the SSIM map }   (device, caller zero-fills)
 *        ssim_maps_opt: [3][items*channels][H][W] partial derivatives kept for the backward pass (NULL: value only)
 *   bwd: dimg = s * ( w_l1 * sign(img-gt) + w_ssim * d(sum SSIM map)/d img ),  s = *grad_scale_dev_opt (device) or 1
 *        (loss = L1 + lambda (1 - ssim)  ->  w_l1 = 1/n, w_ssim = -lambda/n with n = items*channels*H*W)
 * ---------------------------------------------------------------------------------------------------------- */
int fdgs_image_loss_fwd(void* stream, int items, int channels, int H, int W, const float* img, const float* gt,
                        float* ssim_maps_opt, float* acc);
int fdgs_image_loss_bwd(void* stream, int items, int channels, int H, int W, const float* img, const float* gt,
                        const float* ssim_maps, float w_l1, float w_ssim, const float* grad_scale_dev_opt, float* dimg);

/* ------------------------------------------------------------------------------------------------------------
 * HexPlane regulariser: replaces GaussianModel.compute_regulation (scene/gaussian_model.py:538-577 with
 * compute_plane_smoothness of scene/regulation.py:22-28; evaluated at train.py:208-211 every fine iteration).
 *   loss += sum_planes [ w_smooth * mean_{C,H-2,W} (p[h+2] - 2 p[h+1] + p[h])^2 + w_l1 * mean |1 - p| ]
 * The caller passes, per plane, the weight that the reference applies to it: planes (0,1,3) of a level get
 * w_smooth = plane_tv_weight, planes (2,4,5) get w_smooth = time_smoothness_weight and w_l1 = l1_time_planes_weight.
 * Planes are channels-last [H][W][C] device arrays (as in fdgs_deform_params).  One launch computes the value
 * (accumulated into *loss_acc_opt, caller zero-fills) and, for planes with grad_opt != NULL, accumulates
 * grad_scale * (*grad_scale_dev_opt, 1 if NULL) * dloss/dplane into grad_opt (same layout).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct fdgs_reg_plane {
    const float* plane;   /* [H][W][C] */
    float* grad_opt;      /* [H][W][C], accumulated (+=) */
    int H, W, C;
    float w_smooth;       /* weight of the second-difference term (0: skipped) */
    float w_l1;           /* weight of mean |1 - p| (0: skipped) */
} fdgs_reg_plane;
int fdgs_plane_regulation(void* stream, int nplanes, const fdgs_reg_plane* planes /* host array */, float grad_scale,
                          const float* grad_scale_dev_opt, float* loss_acc_opt);

/* ------------------------------------------------------------------------------------------------------------
 * Optimizer step: replaces torch.optim.Adam(l, lr=0.0, eps=1e-15).step() of the reference (scene/gaussian_model.py:184,
 * train.py:291) for all parameter tensors of a step in one launch.  Per tensor: element count, the four device
 * arrays (same memory order, 16-byte aligned), the group's learning rate and the tensor's step count AFTER this step
 * (t >= 1, bias corrections 1 - beta^t).  No weight decay, no amsgrad (the reference uses neither).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct fdgs_adam_tensor {
    float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
    size_t n;
    float lr;
    int step;
} fdgs_adam_tensor;
int fdgs_adam_step(void* stream, int ntensors, const fdgs_adam_tensor* tensors /* host array */, double beta1, double beta2,
                   double eps);   /* doubles: 1 - beta and the bias corrections are formed in double like torch does */

/* Sparse Adam: the same step over [rows, row_len] tensors with a per-tensor row mask (graphdeco's SparseGaussianAdam, gsplat's
 * SelectiveAdam).  Row i with visible[i] != 0 gets exactly the arithmetic of fdgs_adam_step; every other row keeps param, exp_avg and
 * exp_avg_sq bit for bit and its gradient is not looked at (a NaN there changes nothing).  visible == NULL: every row is stepped, so dense
 * and masked tensors of one step share one launch (64 tensors per launch, as fdgs_adam_step).  bias_correction == 0: step_size = lr and
 * sqrt(1 - beta2^t) = 1, the upstream kernels' form.  `step` counts calls per tensor, not visits per row.  Refused before anything is
 * launched: NULL arrays, step < 1, row_len < 1, rows * row_len >= 2^32, arrays that are not 16-byte aligned; ntensors == 0 and
 * rows == 0 are no-ops.  fdgs_adam_step_rows_host: the same over host arrays, without a GPU (the same per-element function). */
typedef struct fdgs_adam_rows_tensor {
    float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
    size_t rows;
    int row_len;
    const unsigned char* visible;   /* NULL = dense, [rows] otherwise */
    float lr;
    int step;
} fdgs_adam_rows_tensor;
int fdgs_adam_step_rows(void* stream, int ntensors, const fdgs_adam_rows_tensor* tensors /* host array */, double beta1, double beta2,
                        double eps, int bias_correction);
int fdgs_adam_step_rows_host(int ntensors, const fdgs_adam_rows_tensor* tensors, double beta1, double beta2, double eps,
                             int bias_correction);

/* ------------------------------------------------------------------------------------------------------------
 * Scale initialisation: replaces simple_knn._C.distCUDA2 (un-vendored submodule submodules/simple-knn, .gitmodules:1-3;
 * call site scene/gaussian_model.py:148).  mean_dist2[i] = mean of the three smallest squared distances from point i
 * to the other points (self excluded by index).  points [N,3], mean_dist2 [N], device.
 * ---------------------------------------------------------------------------------------------------------- */
int fdgs_knn3_mean_dist2(void* stream, int N, const float* points, float* mean_dist2);

/* ------------------------------------------------------------------------------------------------------------
 * Densification bookkeeping (the consumer of render()'s radii / viewspace_points.grad).
 *
 * fdgs_densification_stats: train.py:259-262 + GaussianModel.add_densification_stats (scene/gaussian_model.py:516-518),
 *   for every visible Gaussian (visibility_opt != 0, or radii > 0 when it is NULL):
 *     max_radii2D = max(max_radii2D, radii)   (skipped when max_radii2D_opt is NULL)
 *     xyz_gradient_accum += |viewspace_grad[:, :2]|,  denom += 1            (viewspace_grad rows of grad_stride floats)
 *
 * fdgs_densify_plan / fdgs_densify_apply: GaussianModel.densify (densify_and_clone + densify_and_split,
 *   scene/gaussian_model.py:409-456, 495-500), GaussianModel.prune / prune_points (:350-365, 481-494) with the
 *   optimizer-state surgery of cat_tensors_to_optimizer / _prune_optimizer (:331-348, 367-389).
 *   plan  FDGS_PLAN_DENSIFY: g = accum/denom (NaN -> 0), big = max(exp(scaling)) > dense_size (= percent_dense * extent):
 *                            clone when |g| >= grad_threshold and not big; split (N = 2) when g >= grad_threshold and big
 *         FDGS_PLAN_PRUNE  : drop when sigmoid(opacity) < min_opacity, or (max_screen_size > 0 and (max_radii2D >
 *                            max_screen_size or max(exp(scaling)) > max_world_size (= 0.1 * extent)))
 *         FDGS_PLAN_MASK   : drop where drop_mask != 0 (prune_points(mask))
 *         counts_host[3] = { rows kept, clones, split Gaussians }: the ONE blocking readback (the reference syncs on
 *         .any() / .sum() / boolean indexing many times); N_out = kept + clones + 2 * splits.
 *   apply writes every output row exactly once, order [kept originals | clones | first children | second children];
 *         exp_avg / exp_avg_sq of new rows are 0 (NULL inputs = no optimizer state yet = zeros; NULL outputs = skipped);
 *         side arrays: deformation_table follows its Gaussian, the four statistics survive on kept rows and are 0 on
 *         new rows (any of them may be NULL in `out`).  split_samples: [2*splits][3] standard normals, row
 *         k*splits + r belongs to child k of the r-th split Gaussian (torch.normal over stds.repeat(2,1)); NULL puts
 *         the children on their parent.
 * ---------------------------------------------------------------------------------------------------------- */
#define FDGS_NGROUPS 6          /* xyz, f_dc, f_rest, opacity, scaling, rotation (scene/gaussian_model.py:176-185) */
#define FDGS_PLAN_DENSIFY 0
#define FDGS_PLAN_PRUNE 1
#define FDGS_PLAN_MASK 2
typedef struct {
    int N;                                  /* Gaussians before */
    int width[FDGS_NGROUPS];                /* floats per row: 3, 3, 3*((deg+1)^2-1), 1, 3, 4 (0 = group absent) */
    const float* param[FDGS_NGROUPS];
    const float* exp_avg[FDGS_NGROUPS];
    const float* exp_avg_sq[FDGS_NGROUPS];
    const uint8_t* deformation_table;       /* opt [N] */
    const float* xyz_gradient_accum;        /* opt [N] */
    const float* denom;                     /* opt [N] */
    const float* max_radii2D;               /* opt [N] */
    const float* deformation_accum;         /* opt [N,3] */
} fdgs_gaussians_in;
typedef struct {
    float* param[FDGS_NGROUPS];             /* [N_out][width] */
    float* exp_avg[FDGS_NGROUPS];
    float* exp_avg_sq[FDGS_NGROUPS];
    uint8_t* deformation_table;
    float* xyz_gradient_accum;
    float* denom;
    float* max_radii2D;
    float* deformation_accum;
} fdgs_gaussians_out;

int fdgs_densification_stats(void* stream, int N, const int32_t* radii, const uint8_t* visibility_opt,
                             const float* viewspace_grad, int grad_stride, float* max_radii2D_opt,
                             float* xyz_gradient_accum, float* denom);
int fdgs_densify_scratch_bytes(int N, size_t* bytes);
int fdgs_densify_plan(void* stream, int mode, int N, const float* xyz_gradient_accum, const float* denom,
                      const float* scaling, const float* opacity, const float* max_radii2D, const uint8_t* drop_mask,
                      float grad_threshold, float dense_size, float min_opacity, float max_screen_size,
                      float max_world_size, void* scratch, uint32_t* counts_host);
int fdgs_densify_apply(void* stream, const fdgs_gaussians_in* in, const fdgs_gaussians_out* out, const void* scratch,
                       const float* split_samples_opt);

/* ABI 6: row permutation of per-Gaussian arrays of 4-byte elements that share the row index, in one launch:
 * dst[i] = src[perm[i]] (scatter = 0) or dst[perm[i]] = src[i] (scatter = 1), rows of `width` elements.  `perm` is a permutation of 0 .. N-1
 * (int32, device).  The Python host reads an unordered model's parameters through the cached Hilbert permutation of its positions
 * (fdgs.render) and hands the per-Gaussian gradients back through the inverse. */
#define FDGS_MAX_ROW_ARRAYS 8
typedef struct fdgs_row_array { const void* src; void* dst; int width; } fdgs_row_array;
int fdgs_permute_rows(void* stream, int N, const int32_t* perm, int narrays, const fdgs_row_array* arrays, int scatter);

/* ------------------------------------------------------------------------------------------------------------
 * Spatial order (additions to ABI 6; no existing signature changed): the permutation fdgs_permute_rows needs, produced by the
 * library -- the space-filling-curve key of every position and the STABLE ascending argsort of those keys (csrc/spatial.hip).
 *   key: per axis, lo = min / hi = max of the two bound rows, cell = trunc(clamp((p - lo) / max(hi - lo, 1e-20) * 2^bits, 0, 2^bits - 1))
 *        with the quotient correctly rounded to float32; the three cells go through Skilling's transpose algorithm (Hilbert) or are
 *        interleaved x -> bit 0, y -> bit 1, z -> bit 2 (Morton), spread to the 30-bit layout.  bits = 1 .. 10; a key uses 3 * bits bits.
 *        Bit for bit what fdgs.densify.hilbert_keys / morton_keys compute with torch on the host.
 *   bounds_opt: device float[2][3], two opposite corners of the box in either row order (the reference's HexPlaneField.aabb as it is);
 *        NULL = the bounding box of the points, reduced on the device into `scratch` (no read-back).
 *   scratch: fdgs_spatial_order_scratch_bytes(N) bytes of device memory (contents unspecified before and after; one per stream).
 *        fdgs_spatial_keys needs it only when bounds_opt is NULL.
 *   N = 0 succeeds and writes nothing.  N < 0, bits outside 1 .. 10, an unknown curve or a NULL required pointer return FDGS_E_INVALID
 *   with a message.  A non-finite coordinate is quantised to cell 0 of its axis (and left out of the bounding box).
 *   All launches go on `stream`; nothing synchronises.
 * A raw binding keeps its set ordered like the Python host does: after the set changed, fdgs_spatial_order -> fdgs_permute_rows over every
 * per-Gaussian array (scatter = 0) -> fdgs_deform_grads::spatially_ordered = 1.
 * ---------------------------------------------------------------------------------------------------------- */
#define FDGS_CURVE_HILBERT 0
#define FDGS_CURVE_MORTON  1
/* host-only size query (works without a GPU, like fdgs_geom_bytes) */
int fdgs_spatial_order_scratch_bytes(int N, size_t* bytes);
/* keys[N] (uint32) of xyz[N,3] */
int fdgs_spatial_keys(void* stream, int N, const float* xyz, const float* bounds_opt, int curve, int bits,
                      void* scratch, uint32_t* keys);
/* perm[N] (int32): new row i = old row perm[i] = the STABLE ascending argsort of those keys (equal keys keep their row order);
 * sorted_keys_opt[N] (= keys[perm[i]]) may be NULL */
int fdgs_spatial_order(void* stream, int N, const float* xyz, const float* bounds_opt, int curve, int bits,
                       void* scratch, int32_t* perm, uint32_t* sorted_keys_opt);
/* the same key function evaluated on the HOST over host arrays (bounds_opt NULL = bounding box): diagnostics / tests, no GPU */
int fdgs_spatial_keys_host(int N, const float* xyz, const float* bounds_opt, int curve, int bits, uint32_t* keys);

/* ------------------------------------------------------------------------------------------------------------
 * Playback (additions to ABI 6; no existing signature changed): what rendering a trained model from BAKED states needs beside the
 * rasterizer (csrc/playback.hip).  A baked state is what fdgs_deform_fwd wrote with activate = 1 for one frame time; it depends on the
 * time only, never on the camera, so a sequence is deformed once per timestamp and every later frame is stages 1-4 alone (fdgs.playback).
 * The arithmetic of each operation is one host/device function (csrc/playback_ops.h) compiled without contraction, with IEEE `/` and
 * sqrt: every *_host twin below returns, over host arrays and without a GPU, bit for bit what the device entry point writes.
 * All launches go on `stream`; nothing synchronises.  Bad arguments return FDGS_E_INVALID with a message before anything is launched.
 * ---------------------------------------------------------------------------------------------------------- */
/* Temporal blend of two baked states at weight w in [0, 1] (w = 0: state a), ONE launch for all of it:
 *   flat streams (positions, scales, opacities, SH coefficients; any subset):   out = a + w * (b - a)          element-wise, three roundings
 *   rotations [N,4], unit quaternions in, unit quaternions out (rot_* all NULL: none):
 *        s = dot(a, b) < 0 ? -1 : 1;  q = a + w * (s * b - a);  out = q / max(sqrt(q . q), 1e-12)
 *        (dot product and squared norm summed in index order 0, 1, 2, 3)
 *   `streams` is a HOST array; a, b, out of every stream and the rotations are device pointers, 16-byte aligned (a lane moves 16 bytes;
 *   the n_floats % 4 floats at the end of a stream are handled singly); out overlaps neither a nor b.  A stream with
 *   n_floats = 0 is skipped; nothing to do (N = 0 and no floats) succeeds without a launch.  The *_host twin takes host pointers of any
 *   alignment. */
#define FDGS_MAX_BLEND_STREAMS 4
typedef struct fdgs_blend_stream { const float* a; const float* b; float* out; size_t n_floats; } fdgs_blend_stream;
int fdgs_state_blend(void* stream, float w, int nstreams, const fdgs_blend_stream* streams, int N, const float* rot_a,
                     const float* rot_b, float* rot_out);
int fdgs_state_blend_host(float w, int nstreams, const fdgs_blend_stream* streams, int N, const float* rot_a,
                          const float* rot_b, float* rot_out);
/* The vertex table of a static 3DGS PLY (GaussianModel.save_ply's attribute order) from RAW deformation outputs (activate = 0):
 *   xyz [N,3], scales [N,3], rotations [N,4], opacity [N,1], shs [N,16,3]  ->  out float32 [N,62]:
 *   x y z | nx ny nz (zeros) | f_dc_c = shs[n,0,c] | f_rest_{c * 15 + k} = shs[n,1+k,c] | opacity | scale_0..2 | rot_0..3
 * Pure data movement.  N = 0 succeeds and writes nothing. */
int fdgs_pack_ply_rows(void* stream, int N, const float* xyz, const float* scales, const float* rotations, const float* opacity,
                       const float* shs, float* out);
int fdgs_pack_ply_rows_host(int N, const float* xyz, const float* scales, const float* rotations, const float* opacity,
                            const float* shs, float* out);
/* float32 image [3,H,W] -> uint8 [H,W,3]:
 *   FDGS_RGB8_TRUNC  (uint8)(255.f * min(max(x, 0), 1))                              one rounding, then truncation (the reference's to8b)
 *   FDGS_RGB8_ROUND  t = x * 255.f; t = t + 0.5f; clamp to [0, 255]; truncate        two roundings (torchvision.utils.save_image)
 * The result for a NaN input is unspecified in both modes.  An empty image succeeds and writes nothing. */
#define FDGS_RGB8_TRUNC 0
#define FDGS_RGB8_ROUND 1
int fdgs_image_rgb8(void* stream, int H, int W, int mode, const float* image, uint8_t* out);
int fdgs_image_rgb8_host(int H, int W, int mode, const float* image, uint8_t* out);

/* ------------------------------------------------------------------------------------------------------------
 * Scene composition (additions to ABI 6; no existing signature changed): several baked models in one frame (csrc/compose.hip,
 * fdgs.compose).  Each model is moved into a common world by a PLACEMENT, a similarity transform, and written into its rows of one
 * composite state that is rasterized once -- what the reference's merge_many_4dgs.py does with torch ops and a `cat` per frame.
 * The arithmetic is one host/device function per operation (csrc/compose_ops.h, contraction off, `*` `+` `-` only): the *_host twin
 * returns bit for bit what the device writes.
 *
 *   scale       s > 0, finite
 *   rot         R, row-major 3x3, orthonormal, det +1;   quat = the unit quaternion of R in the rasterizer's (r, x, y, z) order
 *   shift       d
 *   sh1 sh2 sh3 M1 [3x3], M2 [5x5], M3 [7x7], row-major [j][k]: how the coefficients of SH band l mix under R (fdgs.compose.sh_rotation)
 *   mode        FDGS_PLACE_POINTS  the reference script: positions and scales are placed, rotations and SH are copied bit for bit
 *               FDGS_PLACE_RIGID   rotations and SH are turned as well: the placed model looks like the model seen from the moved camera
 *   sh_degree   the model's active SH degree, 0 .. 3
 *
 *   positions   t_k = s * p_k;  y_i = R[i][0] * t_0 + R[i][1] * t_1 + R[i][2] * t_2 (left to right);  out_i = y_i + d_i
 *   scales      out_k = s * scale_k                             (activated scales are lengths)
 *   rotations   RIGID: out = quat (x) q, the Hamilton product, every component four products summed as csrc/compose_ops.h writes them;
 *               not renormalised
 *   opacity     a copy, always
 *   SH [16,3]   per colour channel: band 0 is copied; RIGID: band l = 1 .. 3, out[k] = sum_j in[j] * M_l[j][k], j ascending from +0;
 *               in both modes the bands above sh_degree are written as +0.0 (a model of lower degree is exact inside a composite of a
 *               higher one)
 *
 * When a second state b is given every value is first blended at weight w in [0, 1] exactly as fdgs_state_blend blends it (the same
 * functions), then placed: the result is fdgs_state_blend followed by a placement, bit for bit, in one launch.  b == NULL: no blend,
 * w must be 0.
 *
 * Bit h of field_mask selects field h in the order of fdgs_state_arrays (positions, scales, rotations, opacity, SH); a field that is not
 * selected is neither read nor written and its pointers may be NULL.  a (and b) are the arrays of a baked state: device pointers, the
 * rotations and SH 16-byte aligned.  `out` points at the destination of row 0 of THIS model inside the composite, already offset by the
 * caller: 4-byte alignment is all it needs.  out overlaps neither a nor b.  N = 0 or field_mask = 0 succeed without a launch; otherwise
 * ONE launch on `stream`, the placement passed by value.  The *_host twin takes host pointers of any alignment. */
#define FDGS_PLACE_POINTS 0
#define FDGS_PLACE_RIGID 1
typedef struct fdgs_placement { float scale; float rot[9]; float quat[4]; float shift[3]; float sh1[9]; float sh2[25]; float sh3[49]; int mode; int sh_degree; } fdgs_placement;
typedef struct fdgs_state_arrays { float *xyz, *scales, *rotations, *opacity, *shs; } fdgs_state_arrays;
int fdgs_state_place(void* stream, const fdgs_placement* p, int N, unsigned field_mask, const fdgs_state_arrays* a,
                     const fdgs_state_arrays* b, float w, const fdgs_state_arrays* out);
int fdgs_state_place_host(const fdgs_placement* p, int N, unsigned field_mask, const fdgs_state_arrays* a,
                          const fdgs_state_arrays* b, float w, const fdgs_state_arrays* out);
/* Placing a SPARSE bake (addition to ABI 6; no existing signature changed): fdgs_state_scatter and fdgs_state_place in one launch, for a
 * model of which only D of its N rows move (fdgs.playback.bake_sparse inside fdgs.compose).  For r = 0 .. D-1: row r of the COMPACT arrays
 * a ([D, width]) -- blended with row r of b at weight w when b != NULL -- is placed by p and written to row rows[r] of out; `out` points
 * at row 0 of the model's N rows inside the composite, as for fdgs_state_place.  Rows of out that are not listed and fields that are not
 * selected are not touched.  The listed rows hold, bit for bit, what fdgs_state_place(p, D, field_mask, a, b, w, tmp) writes to tmp,
 * row r moved to row rows[r]: the same functions of csrc/compose_ops.h, nothing else.
 *
 *   rows        a device int32[D], 4-byte aligned, STRICTLY ASCENDING, every entry in [0, N) (the list of the sparse playback entry points)
 *   alignment   every array 4-byte aligned, the rotations and SH of a and b 16-byte aligned; out needs 4 bytes only.  Every row of
 *               out.shs has the alignment of out.shs (192 bytes a row): 16-byte aligned it is stored as float4 pieces, else float by float
 *
 * D = 0, N = 0 or field_mask = 0 succeed without a launch; otherwise ONE launch on `stream`, row name "state_place_rows" in
 * fdgs_timing_report.  FDGS_E_INVALID with a message, before anything is launched or written: what fdgs_state_place refuses (placement,
 * field_mask, w, NULL or misaligned arrays of a selected field), D < 0, N < 0, D > N, rows == NULL or misaligned.  The device entry
 * point cannot inspect `rows`: the kernel compares every index, as an unsigned number, against N and SKIPS a row that fails, so a bad
 * list cannot store out of bounds -- what it does store is unspecified.  The *_host twin takes host pointers of any alignment, validates
 * the list (range, strictly ascending) and returns FDGS_E_INVALID without writing anything. */
int fdgs_state_place_rows(void* stream, const fdgs_placement* p, int D, const int32_t* rows, int N, unsigned field_mask,
                          const fdgs_state_arrays* a, const fdgs_state_arrays* b, float w, const fdgs_state_arrays* out);
int fdgs_state_place_rows_host(const fdgs_placement* p, int D, const int32_t* rows, int N, unsigned field_mask,
                               const fdgs_state_arrays* a, const fdgs_state_arrays* b, float w, const fdgs_state_arrays* out);

/* ------------------------------------------------------------------------------------------------------------
 * Sparse baked playback (additions to ABI 6; no existing signature changed): a baked sequence that keeps ONE full state and, per
 * timestamp, only the rows that move (csrc/playback.hip, fdgs.playback.bake_sparse).  Three operations over fdgs_state_arrays with the
 * field-mask convention of fdgs_state_place: bit h of field_mask selects field h (positions, scales, rotations, opacity, SH); a field
 * that is not selected is neither read nor written and its pointers may be NULL.  The arithmetic is host/device functions of
 * csrc/playback_ops.h compiled without contraction: every *_host twin returns, over host arrays, bit for bit what the device writes.
 *
 *   rows        a device int32[D], STRICTLY ASCENDING, every entry in [0, N)
 *   a, b, compact   arrays of D rows ([D, width]);   full, out, ref, cur   arrays of N rows ([N, width])
 *   alignment   rotations and SH 16-byte aligned on both sides (a lane moves 16 bytes), positions, scales and opacity 4-byte aligned;
 *               the *_host twins take host pointers of any alignment
 *   out overlaps neither a nor b
 *
 * D = 0, N = 0 or field_mask = 0 succeed without a launch; otherwise ONE launch on `stream`, nothing synchronises.  FDGS_E_INVALID with a
 * message, before anything is launched or written: a NULL required pointer; D < 0, N < 0 or D > N; w outside [0, 1] or NaN;
 * b == NULL with w != 0; a field_mask above 31; a misaligned rotation or SH pointer (device entry points).
 * The device entry points cannot inspect `rows`: the kernels compare every row index, as an unsigned number, against N and SKIP a row
 * that fails, so a bad list cannot store (or load) out of bounds -- what it does store is unspecified.  The *_host twins validate the
 * list (range, strictly ascending) and return FDGS_E_INVALID without writing anything. */
/* extent[n][h] (float32 [N,5], caller zero-fills before the first call) = running maximum, over calls and over the components c of
 * field h in ascending order, of |cur_h[n][c] - ref_h[n][c]|:   d = cur - ref;  m = fabsf(d);  m != m ? e = +inf : (m > e ? e = m : e)
 * (a NaN difference -- a NaN component, inf - inf -- makes the extent +inf).  Columns of unselected fields are left untouched.
 * One launch. */
int fdgs_state_extent(void* stream, int N, unsigned field_mask, const fdgs_state_arrays* ref, const fdgs_state_arrays* cur, float* extent);
int fdgs_state_extent_host(int N, unsigned field_mask, const fdgs_state_arrays* ref, const fdgs_state_arrays* cur, float* extent);
/* compact_h[r] = full_h[rows[r]], r = 0 .. D-1: bit copies.  One launch. */
int fdgs_state_gather(void* stream, int D, const int32_t* rows, int N, unsigned field_mask, const fdgs_state_arrays* full,
                      const fdgs_state_arrays* compact);
int fdgs_state_gather_host(int D, const int32_t* rows, int N, unsigned field_mask, const fdgs_state_arrays* full,
                           const fdgs_state_arrays* compact);
/* out_h[rows[r]] = a_h[r] (b == NULL, w must be 0: bit copies) or the blend of a_h[r] and b_h[r] at weight w in [0, 1], by blend_lerp /
 * blend_quat of playback_ops.h, i.e. exactly what fdgs_state_blend writes for those two rows.  Rows of `out` that are not listed are
 * not touched.  One launch. */
int fdgs_state_scatter(void* stream, int D, const int32_t* rows, int N, unsigned field_mask, const fdgs_state_arrays* a,
                       const fdgs_state_arrays* b, float w, const fdgs_state_arrays* out);
int fdgs_state_scatter_host(int D, const int32_t* rows, int N, unsigned field_mask, const fdgs_state_arrays* a,
                            const fdgs_state_arrays* b, float w, const fdgs_state_arrays* out);

/* ------------------------------------------------------------------------------------------------------------
 * Motion vectors and coverage (additions to ABI 6; no existing signature changed): the two small launches around ONE extra blend pass of
 * a finished forward-only frame (csrc/motion.hip, fdgs.playback.Baked.render_motion; see fdgs_geom_field for why the second
 * fdgs_render_fwd is valid).  The arithmetic is host/device functions of csrc/motion_ops.h compiled without contraction: every *_host
 * twin returns, over host arrays, bit for bit what the device writes.
 * ---------------------------------------------------------------------------------------------------------- */
/* Row n of `out` = (mx, my, 1): where the point xyz_at[n], seen through (view_at, proj_at), is in the image of (view_toward, proj_toward)
 * once it has moved to xyz_toward[n], minus where it is now, in pixels of a W x H image (the rasterizer's pixel convention).  ADD it to a
 * pixel's coordinates in this frame to find the same surface point in the toward frame.  A row whose view-space depth is <= 0.2 (the
 * rasterizer's near cull) in EITHER view gets (0, 0, 1).  The third float is always 1: blended, it is the coverage.
 * out_stride = 3 or 4 floats per row; with 4 the fourth float is written as +0 (a recC record).  xyz_* and out need 4-byte alignment
 * only (row slices are fine); a 16-byte aligned out with stride 4 is written one float4 per row.  The four matrices are [16] each, device.
 * N = 0 succeeds without a launch, otherwise ONE launch; FDGS_E_INVALID with a message for a NULL pointer, N < 0, another stride, W or H < 1. */
int fdgs_motion_rows(void* stream, int N, const float* xyz_at, const float* xyz_toward, const float* view_at, const float* proj_at,
                     const float* view_toward, const float* proj_toward, int W, int H, float* out, int out_stride);
int fdgs_motion_rows_host(int N, const float* xyz_at, const float* xyz_toward, const float* view_at, const float* proj_at,
                          const float* view_toward, const float* proj_toward, int W, int H, float* out, int out_stride);
/* raw [3,H,W] = the blend of the rows above over a zero background.  Per pixel, with a = raw[2]: motion [2,H,W] = raw[0..1] / a where
 * a > min_alpha, 0 elsewhere (a NaN a gives zeros); alpha [1,H,W] = a, a copy.  One launch. */
int fdgs_motion_resolve(void* stream, int H, int W, float min_alpha, const float* raw, float* motion, float* alpha);
int fdgs_motion_resolve_host(int H, int W, float min_alpha, const float* raw, float* motion, float* alpha);

/* ------------------------------------------------------------------------------------------------------------
 * Pick pass (an addition to ABI 6; no existing signature changed): which Gaussian a pixel of a finished frame shows and the depth at
 * which the pixel turns opaque, from ONE more walk over the frame's own sorted lists (csrc/render.hip: render_pick_kernel,
 * fdgs.playback.Baked.render_pick).  No second projection, no sort.  An argmax and a threshold crossing are not linear in a colour, so
 * this is not a second fdgs_render_fwd (what the motion pass is) but a kernel of its own.
 *
 * Valid after fdgs_render_fwd, or after fdgs_raster_fwd_capacity once the frame is known to be exact (true count <= capacity), with the
 * same geom, binning and img and the num_rendered the buffers were laid out for; a training frame or a forward-only one.  Per pixel the
 * tile's list is walked from the front up to the pixel's n_contrib with exactly the forward's decisions -- the power, alpha =
 * min(0.99, opacity * exp(power)), the power > 0 and alpha < 1/255 skips, w = alpha * T, T *= 1 - alpha are the forward's expressions:
 * w has the bits of the weight the forward blended the Gaussian's colour with -- and A is the float32 running sum of w in list order
 * (what a blended colour channel of ones accumulates).
 * -------------------------------------------------------------------------------------------------------- */
typedef struct fdgs_pick_out {
    int32_t* pick_id;       /* opt [H*W]: the Gaussian with the largest w (a tie goes to the earlier list entry, the one in front); -1 where
                               nothing contributed */
    float*   pick_weight;   /* opt [H*W]: that w; +0 where nothing contributed */
    int32_t* surface_id;    /* opt [H*W]: the first contributor after whose w was added A >= alpha_cut holds; -1 where A never gets there */
    float*   surface_depth; /* opt [H*W]: that contributor's view depth (recB.z, the value the forward blends into out_depth); +0 where
                               surface_id is -1 */
} fdgs_pick_out;
/* alpha_cut in (0, 1] (0.5: the median depth).  row_map_opt: device int32[P] or NULL; when given, an id g is written as row_map_opt[g]
 * (-1 stays -1): ids in another row order than the one the rasterizer was handed.  Any output may be NULL, not all four.
 * FDGS_E_INVALID with a message, before anything is launched, for: a NULL params, geom, binning, img or out; W or H < 1; an alpha_cut
 * outside (0, 1] or NaN; all four outputs NULL; an output or row_map_opt that is not 4-byte aligned.  P == 0 or num_rendered == 0
 * succeeds and writes -1 / +0 everywhere.  ONE launch on `stream`, nothing synchronises (params->debug aside); its row in
 * fdgs_timing_report is "render_pick".
 * It WRITES NOTHING into geom, binning or img: final_T, n_contrib, the ranges, the walk lengths and the tile orders keep their bits (the
 * tiles are taken in the order the forward left in img field 4, which is read, not rebuilt), so a motion pass or fdgs_raster_bwd of the
 * same frame may follow.  A stale img cannot make it read past a list: every walk is clamped to the tile's range and num_rendered. */
int fdgs_render_pick(void* stream, const fdgs_raster_params* p, const void* geom, const void* binning, const void* img,
                     uint32_t num_rendered, float alpha_cut, const int32_t* row_map_opt, const fdgs_pick_out* out);

/* ------------------------------------------------------------------------------------------------------------
 * Contribution pass (an addition to ABI 6; no existing signature changed): how much every Gaussian adds to a finished frame -- the inverse
 * of the pick pass's question --, from ONE more walk over the frame's own sorted lists (csrc/render.hip: render_contrib_kernel,
 * fdgs.playback.Baked.render_contrib).  No second projection, no sort.  The per-Gaussian sum of w = alpha * T is decided inside the
 * blend and is not linear in a per-Gaussian colour, so this is not a second fdgs_render_fwd but a kernel of its own.
 *
 * Valid wherever fdgs_render_pick is valid, with the same geom, binning, img and num_rendered.  Per pixel the tile's list is walked from
 * the front up to the pixel's n_contrib with exactly the forward's decisions and expressions (the pick pass's walk: w has the bits of
 * the weight the forward blended the Gaussian's colour with).  v = w, or with a pixel weight v = w * pixel_weight_opt[pixel] as ONE
 * rounded product.  A pixel or entry with !(v > 0) is skipped entirely -- a zero, negative or NaN weight is neither summed, maxed nor
 * counted.
 * -------------------------------------------------------------------------------------------------------- */
typedef struct fdgs_contrib_row {   /* 16 bytes, one per Gaussian; ACCUMULATED into, never cleared by the call */
    float    weight_sum;   /* += sum over pixels of v (float32; the order of the additions across tiles is not fixed) */
    float    weight_max;   /* = max(old, max over pixels of v): exact */
    uint32_t pixels;       /* += number of pixels with v > 0: exact */
    uint32_t tiles;        /* += number of 16 x 16 tiles in which at least one pixel had v > 0: exact */
} fdgs_contrib_row;
/* rows: device fdgs_contrib_row[P], 16-byte aligned; zero it before the first pass, accumulate any number of frames (views, times) into
 * it.  Gaussian g goes to rows[row_map_opt ? row_map_opt[g] : g] (row_map_opt: device int32[P] or NULL); an id outside [0, P), before
 * or after the map, is dropped.  pixel_weight_opt: device float[H*W] or NULL (a lasso, a mask, a saliency map).
 * FDGS_E_INVALID with a message, before anything is launched, for: a NULL params, geom, binning, img or rows; W or H < 1; P < 0; rows
 * not 16-byte aligned; pixel_weight_opt or row_map_opt not 4-byte aligned.  P == 0 or num_rendered == 0 succeeds without touching
 * rows (and without a launch).  Otherwise ONE launch on `stream`, nothing synchronises (params->debug aside); its row in
 * fdgs_timing_report is "render_contrib".  At most one atomic per word of a record and (tile, list entry): f32 add, u32 max on the
 * float's bits (valid because v >= +0), u32 add, u32 add of 1.
 * It WRITES NOTHING into geom, binning or img (the tiles are taken in the order the forward left in img field 4, which is read, not
 * rebuilt), so a pick, a motion pass or fdgs_raster_bwd of the same frame may follow.  A stale img cannot make it read past a list:
 * every walk is clamped to the tile's range and num_rendered. */
int fdgs_render_contrib(void* stream, const fdgs_raster_params* p, const void* geom, const void* binning, const void* img,
                        uint32_t num_rendered, const float* pixel_weight_opt, const int32_t* row_map_opt, fdgs_contrib_row* rows);

/* ------------------------------------------------------------------------------------------------------------
 * Feature pass (an addition to ABI 6; no existing signature changed): C per-row channels of any meaning -- a per-model indicator, a
 * per-row statistic, a label, a normal, an embedding -- blended into [C,H,W] images by ONE more walk over a finished frame's own sorted
 * lists (csrc/render.hip: render_features_kernel, fdgs.playback.Baked.render_features).  No second projection, no sort.  The other way
 * to blend something that is not the model's colour is to overwrite recC of a forward-only frame three channels at a time and call
 * fdgs_render_fwd again (see fdgs_geom_field): one whole blend per three channels, the frame's colours are gone, and a training frame
 * does not allow it.  This kernel evaluates alpha, T and w once per (pixel, entry) and chunk of sixteen channels and reads the values
 * from the caller's own array.
 *
 * Valid wherever fdgs_render_pick is valid, with the same geom, binning, img and num_rendered.  Per pixel the tile's list is walked from
 * the front up to the pixel's n_contrib with exactly the forward's decisions and expressions (the pick pass's walk: w has the bits of
 * the weight the forward blended the Gaussian's colour with).  Channel c of the pixel is the sum over its contributors, in list order,
 * of values[row * value_stride + c] * w with row = row_map_opt ? row_map_opt[g] : g, accumulated as ONE fused multiply-add per entry
 * -- what the forward's colour sums are compiled to --: features[c] has the bits fdgs_render_fwd would write for that channel over a
 * zero background.  A is the float32 running sum of w in list order (the pick pass's; the blend of a channel of ones).  A Gaussian whose
 * row is outside [0, rows) -- a -1 of the map included -- blends as zeros.  No background is added.
 * -------------------------------------------------------------------------------------------------------- */
/* values: device float, row r at values + r * value_stride, value_stride >= C floats; rows: how many rows it has.  Only 4-byte alignment
 * is required of it (a row slice [:, a:a+C] of a wider array is legal); 16-byte loads are used where an address allows them.
 * row_map_opt: device int32[P] or NULL.  features: device float[C*H*W], plane c at features + c * H * W.  alpha_opt: device float[H*W]
 * or NULL, = A.  min_alpha < 0 or NaN: features holds the raw sums.  min_alpha >= 0: features[c] = sum / A (IEEE division, as
 * fdgs_motion_resolve's) where A > min_alpha and +0 elsewhere (a NaN A gives +0); alpha_opt is A either way.
 * FDGS_E_INVALID with a message, before anything is launched, for: a NULL params, geom, binning, img, values or features; W or H < 1;
 * C < 1 or C > 8 * 65535; value_stride < C; rows < 0; values, row_map_opt, features or alpha_opt not 4-byte aligned.  P == 0 or
 * num_rendered == 0 succeeds and writes +0 everywhere, without reading the frame.  ONE launch on `stream` for any C (the channels go in
 * chunks of sixteen, one workgroup per tile and chunk), nothing synchronises (params->debug aside); its row in fdgs_timing_report is
 * "render_features".
 * It WRITES NOTHING into the frame -- geom, binning and img keep their bits, no atomics; the tiles are taken in the order the forward left
 * in img field 4, which is read, not rebuilt --, so a pick, contribution or motion pass, or fdgs_raster_bwd, may follow.  A stale img
 * cannot make it read past a list: every walk is clamped to the tile's range, the tile's walk length and num_rendered. */
int fdgs_render_features(void* stream, const fdgs_raster_params* p, const void* geom, const void* binning, const void* img,
                         uint32_t num_rendered, int C, const float* values, int value_stride, int rows,
                         const int32_t* row_map_opt, float min_alpha, float* features /* [C,H,W] */, float* alpha_opt /* [H,W] */);

/* ------------------------------------------------------------------------------------------------------------
 * Feature pass backward (an addition to ABI 6; no existing signature changed): the adjoint of fdgs_render_features with respect to its
 * values -- what a method that freezes a trained model and optimises one embedding, label or identity per Gaussian against 2-D masks or
 * feature maps needs for a training step -- by ONE more walk over the same finished frame's sorted lists (csrc/render_features_bwd.h:
 * render_features_bwd_kernel, fdgs.playback.Baked.render_features(differentiable=True)):
 *
 *     dvalues[row * dvalue_stride + c] += sum over the pixels of w(row, pixel) * dL_dfeatures[c, pixel]
 *
 * with the w of the forward: the same walk, decisions and expressions (the pick pass's), so w has the bits the forward multiplied the
 * values with.  The sum over a tile's 256 pixels is a contraction on the matrix cores (v_mfma_f32_16x16x4_f32: float32 products and
 * sums, no reduced-precision operand); the order of the additions inside a tile and across tiles is not fixed.  For a normalised forward
 * (min_alpha >= 0) a pixel's gradient is scaled on load, dL_dfeatures[c, pixel] / A (IEEE division) where A = alpha_opt[pixel] >
 * min_alpha and 0 elsewhere.  This is the gradient with respect to `values` ONLY: the path through A, like every other path into the
 * geometry, is not followed (a bake has no live geometry to receive it).
 * A NON-FINITE dL_dfeatures IS OUT OF CONTRACT: the contraction multiplies the zero weights of a tile's skipped entries with every
 * gradient of the wave's 64 pixels, so one inf or NaN reaches (0 * inf) rows that do not contribute to its pixel.
 *
 * Valid wherever fdgs_render_features is valid, with the same geom, binning, img and num_rendered -- for as long as those buffers still
 * hold the frame.  OF *p ONLY P, W, H AND debug ARE READ, AND NONE OF ITS POINTERS IS DEREFERENCED OR COPIED: by the time a backward
 * runs, a later fdgs_state_at may have overwritten the states the frame was projected from; what the walk needs lives in geom, binning
 * and img.
 * -------------------------------------------------------------------------------------------------------- */
/* dL_dfeatures: device float[C*H*W], plane c at dL_dfeatures + c * H * W.  alpha_opt: device float[H*W], the alpha image that forward
 * wrote; required when min_alpha >= 0, not read otherwise (min_alpha < 0 or NaN: the forward wrote raw sums).
 * dvalues: device float, row r at dvalues + r * dvalue_stride, dvalue_stride >= C floats; ACCUMULATED into, never cleared by the call
 * (like fdgs_contrib_row): zero it before the first pass, accumulate any number of frames.  Gaussian g goes to row row_map_opt ?
 * row_map_opt[g] : g (row_map_opt: device int32[P] or NULL); a row outside [0, rows) -- a -1 of the map included -- is dropped.  Only
 * 4-byte alignment is required of it; where rows are 64-byte aligned one atomic instruction covers whole rows.  Floats of a row behind
 * its C channels are not touched.
 * FDGS_E_INVALID with a message, before anything is launched, for: a NULL params, geom, binning, img, dL_dfeatures or dvalues; W or H
 * < 1; C < 1 or C > 8 * 65535; dvalue_stride < C; rows < 0; min_alpha >= 0 with a NULL alpha_opt; dL_dfeatures, alpha_opt, row_map_opt
 * or dvalues not 4-byte aligned.  P == 0 or num_rendered == 0 succeeds without touching dvalues (and without a launch).  Otherwise ONE
 * launch on `stream` for any C (chunks of sixteen channels, one workgroup per tile and chunk), nothing synchronises (params->debug
 * aside); its row in fdgs_timing_report is "render_features_bwd".  At most one float atomic per (tile, list entry, channel); a zero sum
 * issues none, so a row no pixel shows keeps its bits.
 * It WRITES NOTHING into the frame -- geom, binning and img keep their bits; the tiles are taken in the order the forward left in img
 * field 4, which is read, not rebuilt --, so it may run any number of times, before or after a pick, contribution or motion pass.  A
 * stale img cannot make it read past a list: every walk is clamped to the tile's range, the tile's walk length and num_rendered. */
int fdgs_render_features_bwd(void* stream, const fdgs_raster_params* p, const void* geom, const void* binning, const void* img,
                             uint32_t num_rendered, int C, const float* dL_dfeatures /* [C,H,W] */,
                             const float* alpha_opt /* [H,W], required when min_alpha >= 0 */, float min_alpha,
                             const int32_t* row_map_opt, int rows, float* dvalues, int dvalue_stride);

/* ------------------------------------------------------------------------------------------------------------
 * MCMC densification, host side (additions to ABI 6; no existing struct or signature changed): the arithmetic of the second
 * densification strategy beside clone / split / prune -- 3DGS-MCMC (Kheradmand et al. 2024): dead Gaussians are RELOCATED onto live ones
 * sampled by opacity, the set GROWS 5 % at a time up to an exact cap, and every iteration adds opacity-gated, covariance-shaped NOISE to
 * the positions.  csrc/mcmc_ops.h holds one __host__ __device__ function per operation; the functions declared here evaluate them over
 * HOST arrays, without a GPU.  The device kernels and the Python strategy are not part of the library yet.
 * Neither the authors' code nor gsplat's MCMCStrategy is part of the reference tree: THE FORMULAS BELOW ARE THE SPECIFICATION
 * (parity unpinned).  All quantities are canonical (undeformed).
 *
 * Per Gaussian x_o, x_s[3], q[4] are the raw parameters, o = sigmoid(x_o), s = exp(x_s), R(q) the rotation of the normalised quaternion.
 *
 * Dead.  A row is dead when 1 / (1 + expf(-x_o)) <= min_opacity in float32 (the expression of the prune plan; a NaN is dead too).
 *
 * Sampling: with replacement, probability proportional to opacity, over the live rows, exact and independent of any reduction order.
 *   weight[i]  uint32: 0 for a dead row, else clamp(floor(o * 2^32), 1, 2^32 - 1)        (o in float32; o * 2^32 is exact)
 *   scan[i]    uint64 inclusive sum of the weights; total = scan[N - 1]
 *   draw k     (w0, w1, w2, w3) = Philox4x32-10(counter = (k, 0, 0, 0), key = (seed, tag)); u_k = w1 * 2^32 + w0;
 *              r_k = mulhi64(u_k, total) = floor(u_k * total / 2^64); the source is the first row i with scan[i] > r_k.
 *   tag        FDGS_MCMC_TAG_RELOCATE / FDGS_MCMC_TAG_GROW tell the two calls of one refinement apart (the noise has its own, below).
 *   Philox4x32-10 is the generator of Salmon et al. (SC'11): ten rounds of
 *     (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),  M0 = 0xD2511F53, M1 = 0xCD9E8D57,
 *   the key raised by (0x9E3779B9, 0xBB67AE85) after every round.
 *   Replicas with equal parameters and an equal seed draw the same sources without a broadcast.
 *
 * Relocation values of a source drawn c >= 1 times: ratio r = min(c + 1, FDGS_MCMC_MAX_RATIO),
 *   o' = 1 - (1 - o)^(1/r)
 *   D  = sum_{i=1..r} sum_{k=0..i-1} C(i-1, k) (-1)^k o'^(k+1) / sqrt(k+1)
 *   s' = s o / D;   then o' is clamped to [min_opacity, 1 - 2^-23];   x_o' = log(o' / (1 - o')),  x_s' = log(s').
 *   r Gaussians (o', s') at one place blend to the same central alpha, 1 - (1 - o')^r = o, and cover the same area under the alpha
 *   profile as the one (o, s) did; r = 1 is the identity.  The sum alternates with binomials up to C(50, 25) = 1.3e14: the whole chain,
 *   from the raw parameters to x_o' and x_s', is evaluated in DOUBLE and rounded to float32 once (binomials from a constant table; the
 *   inner sums closed by sum_{i=k+1..r} C(i-1, k) = C(r, k+1)).  Where the lower clamp acts, x_o' is rounded UP by between 0.75 and
 *   1.75 units, so that the float32 dead test does not call a row filled with it dead again.
 *
 * Noise: xyz += (R diag(s^2) R^T) xi * g * lr,  g = 1 / (1 + exp(k_gate (o - min_opacity))), evaluated in DOUBLE from the float32 inputs
 *   and rounded by the final add (a float32 rotation matrix carries absolute errors of 2^-24 that the largest s^2 multiplies);
 *   xi ~ N(0, I3): (w0 .. w3) = Philox4x32-10(counter = (row, iteration, 0, 0), key = (seed, FDGS_MCMC_TAG_NOISE));
 *   (xi0, xi1) = sqrt(-2 ln u1) (cos, sin)(2 pi u2), u1 = (w0 + 1) 2^-32 (never 0), u2 = (w1 >> 8) 2^-24; xi2 = the cosine branch of
 *   (w2, w3).  lr = noise_lr * lr_xyz is the caller's product.
 *
 * FDGS_E_INVALID with a message for a negative size or a NULL required pointer (and a scan without a live row); a size of 0 succeeds and
 * touches nothing.
 * ---------------------------------------------------------------------------------------------------------- */
#define FDGS_MCMC_TAG_RELOCATE 0x52454C4Fu /* "RELO" */
#define FDGS_MCMC_TAG_GROW 0x47524F57u     /* "GROW" */
#define FDGS_MCMC_TAG_NOISE 0x4E4F4953u    /* "NOIS" */
#define FDGS_MCMC_MAX_RATIO 51
/* words[i] = Philox4x32-10(counters[i], key = (key0, key1)) */
int fdgs_mcmc_philox_host(int n, const uint32_t* counters /* [n,4] */, uint32_t key0, uint32_t key1, uint32_t* words /* [n,4] */);
/* weights and their inclusive scan from raw opacities */
int fdgs_mcmc_weights_host(int N, const float* opacity, float min_opacity, uint32_t* weights, uint64_t* scan);
/* n draws over a scan; counts_opt[N] (zeroed first) receives the draws per source */
int fdgs_mcmc_sample_host(int N, const uint64_t* scan, int n, uint32_t seed, uint32_t tag, int32_t* src_out, uint32_t* counts_opt /* [N] */);
/* x_o', x_s' of n rows drawn counts[i] times each (0: ratio 1) */
int fdgs_mcmc_relocation_host(int n, const float* opacity, const float* scaling /* [n,3] */, const uint32_t* counts, float min_opacity,
                              float* opacity_out, float* scaling_out);
/* the normals of rows 0 .. N-1 for (seed, iteration) */
int fdgs_mcmc_normals_host(int N, uint32_t seed, uint32_t iteration, float* out /* [N,3] */);
/* the noise step in place on xyz; normals_opt [N,3] replaces the generator's */
int fdgs_mcmc_noise_host(int N, float* xyz, const float* scaling, const float* rotation, const float* opacity, float lr, float k_gate,
                         float min_opacity, uint32_t seed, uint32_t iteration, const float* normals_opt);

#ifdef __cplusplus
}
#endif
#endif /* FDGS_H */
