// raster.h -- the host functions the rasterizer's units call across each other (preprocess.hip, binning.hip, render.hip; spatial.hip
// borrows the sort), declared once.
#pragma once
#include "common.h"

namespace fdgs {

int validate_raster_params(const fdgs_raster_params* p);      // preprocess.hip

// LSD radix sort of n (key,val) pairs over bits [0,nbits) (binning.hip).  Ping-pongs between (k0,v0) and (k1,v1); returns which
// buffer holds the result (0 or 1) through *result_in.
int radix_sort_pairs(hipStream_t stream, uint32_t* k0, uint32_t* v0, uint32_t* k1, uint32_t* v1, uint32_t n, int nbits,
                     uint32_t* hist, int nblocks, int debug, int* result_in, int items = SORT_ITEMS, const uint32_t* n_dev = nullptr);

// does the one-call frame of this image count the tiles' pairs in its projection kernel (knob bin_count; binning.hip)?
bool counts_in_projection(const ImgLayout& il);

// One launch (render.hip): the scan of the tiles' pair counts into img's `ranges` (tile_walk.h: tile_scan_body, cap as there) and, where
// the blending takes its tiles heaviest-first, the forward's tile order from the same counts.  *order_made: the order stands in img.
int launch_tile_scan_order(hipStream_t stream, const ImgLayout& il, const uint32_t* counts, void* img, uint32_t cap, int debug, bool* order_made);

// fdgs_render_fwd / fdgs_render_fwd_alpha; order_made: the forward's tile order already stands in img (launch_tile_scan_order), no launch
// makes it; out_alpha: opt [H*W], the accumulated opacity
int render_fwd_impl(void* stream_, const fdgs_raster_params* p, const void* geom, const void* binning, void* img, uint32_t R, float* out_color,
                    float* out_depth, bool order_made, float* out_alpha);

}  // namespace fdgs

// the projection launchers (preprocess.hip).  host_count_dev (capacity mode): device address of the pinned host word that receives the
// pair count from the kernel's last workgroup.  count_tiles (one-call frame, counts_in_projection): the kernel also counts the pairs of
// every tile into geom's tile_counts, cleared by the same fill as the header in front of them.  antialiasing (the *_aa entry points): the
// projection writes opacity * h into recB.y, and the backward of such a state carries h's chain rule (gs_math.h aa_comp / aa_bwd).
// means2D_abs (fdgs_raster_bwd_abs): opt [P,3], the absolute screen-space sums of the accumulator line, one row per Gaussian
int fdgs_preprocess_fwd_impl(void* stream_, const fdgs_raster_params* p, void* geom, int32_t* radii, uint32_t* host_count_dev,
                             bool count_tiles = false, bool antialiasing = false);
int fdgs_launch_preprocess_bwd(hipStream_t stream, const fdgs_raster_params* p, const void* geom, const fdgs_raster_grads* g,
                               bool antialiasing = false, float* means2D_abs = nullptr);
