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

}  // namespace fdgs

// the projection launchers (preprocess.hip).  host_count_dev (capacity mode): device address of the pinned host word that receives the
// pair count from the kernel's last workgroup
int fdgs_preprocess_fwd_impl(void* stream_, const fdgs_raster_params* p, void* geom, int32_t* radii, uint32_t* host_count_dev);
int fdgs_launch_preprocess_bwd(hipStream_t stream, const fdgs_raster_params* p, const void* geom, const fdgs_raster_grads* g);
