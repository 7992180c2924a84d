// mcmc.hip -- MCMC densification (3DGS-MCMC, Kheradmand et al. 2024): the HOST entry points of its arithmetic.  include/fdgs.h ("MCMC
// densification") states the definitions; mcmc_ops.h holds one __host__ __device__ function per operation -- Philox4x32-10, the integer
// sampling weights, the draw, the relocation values (double), the Box-Muller normals, the noise step (double) -- and the functions below
// evaluate them over host arrays, without a GPU.  The device kernels that call the same functions are not part of the library yet.
#include "common.h"
#include "mcmc_ops.h"

using namespace fdgs;

// ---- host twins (no GPU): the functions of mcmc_ops.h over host arrays ---------------------------------------------------------------------
extern "C" int fdgs_mcmc_philox_host(int n, const uint32_t* counters, uint32_t key0, uint32_t key1, uint32_t* words) {
    FDGS_REQUIRE(n >= 0, "bad sizes");
    if (n == 0) return FDGS_OK;
    FDGS_REQUIRE(counters && words, "NULL pointer");
    for (size_t i = 0; i < (size_t)n; i++)
        philox4x32_10(counters[4 * i], counters[4 * i + 1], counters[4 * i + 2], counters[4 * i + 3], key0, key1, words + 4 * i);
    return FDGS_OK;
}

extern "C" int fdgs_mcmc_weights_host(int N, const float* opacity, float min_opacity, uint32_t* weights, uint64_t* scan) {
    FDGS_REQUIRE(N >= 0, "bad sizes");
    if (N == 0) return FDGS_OK;
    FDGS_REQUIRE(opacity && weights && scan, "NULL pointer");
    uint64_t run = 0;
    for (size_t i = 0; i < (size_t)N; i++) {
        weights[i] = mcmc_weight(opacity[i], min_opacity);
        run += weights[i];
        scan[i] = run;
    }
    return FDGS_OK;
}

extern "C" int fdgs_mcmc_sample_host(int N, const uint64_t* scan, int n, uint32_t seed, uint32_t tag, int32_t* src_out, uint32_t* counts_opt) {
    FDGS_REQUIRE(N >= 0 && n >= 0, "bad sizes");
    if (N == 0 || n == 0) return FDGS_OK;
    FDGS_REQUIRE(scan && src_out, "NULL pointer");
    FDGS_REQUIRE(scan[N - 1] > 0, "no live row to draw from");
    if (counts_opt) memset(counts_opt, 0, (size_t)N * 4);
    for (int k = 0; k < n; k++) {
        src_out[k] = mcmc_draw(N, scan, scan[N - 1], seed, tag, (uint32_t)k);
        if (counts_opt) counts_opt[src_out[k]]++;
    }
    return FDGS_OK;
}

extern "C" int fdgs_mcmc_relocation_host(int n, const float* opacity, const float* scaling, const uint32_t* counts, float min_opacity,
                                         float* opacity_out, float* scaling_out) {
    FDGS_REQUIRE(n >= 0, "bad sizes");
    if (n == 0) return FDGS_OK;
    FDGS_REQUIRE(opacity && scaling && counts && opacity_out && scaling_out, "NULL pointer");
    for (size_t i = 0; i < (size_t)n; i++) mcmc_relocation(opacity[i], scaling + 3 * i, counts[i], min_opacity, opacity_out + i, scaling_out + 3 * i);
    return FDGS_OK;
}

extern "C" int fdgs_mcmc_normals_host(int N, uint32_t seed, uint32_t iteration, float* out) {
    FDGS_REQUIRE(N >= 0, "bad sizes");
    if (N == 0) return FDGS_OK;
    FDGS_REQUIRE(out, "NULL pointer");
    for (size_t i = 0; i < (size_t)N; i++) mcmc_normals3(seed, (uint32_t)i, iteration, out + 3 * i);
    return FDGS_OK;
}

extern "C" int fdgs_mcmc_noise_host(int N, float* xyz, const float* scaling, const float* rotation, const float* opacity, float lr, float k_gate,
                                    float min_opacity, uint32_t seed, uint32_t iteration, const float* normals_opt) {
    FDGS_REQUIRE(N >= 0, "bad sizes");
    if (N == 0) return FDGS_OK;
    FDGS_REQUIRE(xyz && scaling && rotation && opacity, "NULL pointer");
    for (size_t i = 0; i < (size_t)N; i++) {
        float z[3];
        if (normals_opt) { z[0] = normals_opt[3 * i]; z[1] = normals_opt[3 * i + 1]; z[2] = normals_opt[3 * i + 2]; }
        else mcmc_normals3(seed, (uint32_t)i, iteration, z);
        mcmc_noise_row(xyz + 3 * i, scaling + 3 * i, rotation + 4 * i, opacity[i], z, lr, k_gate, min_opacity, xyz + 3 * i);
    }
    return FDGS_OK;
}
