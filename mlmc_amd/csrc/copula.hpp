// What the sampling entries share (density.hip, copula.hip): the uniform numbers of a stream, and the launchers of the Gaussian
// copula's kernels (copula.hip), which the host path of mlmc_density_sample_joint_batch (density.hip) calls.
#pragma once
#include "common.hpp"

namespace mlmc {

// uniform `idx` of stream `stream` under `seed` (include/mlmc_hip.h): Philox counter (idx >> 1, stream, "SAMP"), words (r0, r1) for
// an even idx and (r2, r3) for an odd one, their top 52 bits m, u = (2 m + 1) 2^-53: exact, 0 < u < 1, and 1 - u is exact
__device__ __forceinline__ double q_uniform(uint64_t seed, uint32_t stream, uint64_t idx) {
    const uint64_t i = idx >> 1;
    uint32_t c[4] = {(uint32_t)i, (uint32_t)(i >> 32), stream, 0x53414D50u};
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);         // keyed as bs_philox (bootstrap.hip) and philox_u64 (select.hip)
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    const uint32_t hi = (idx & 1) ? c[2] : c[0], lo = (idx & 1) ? c[3] : c[1];
    const uint64_t m = ((uint64_t)hi << 20) | (uint64_t)(lo >> 12);
    return (double)(int64_t)(2 * m + 1) * 0x1p-53;
}

// Z[k * ldz + c] = latent normal k of draw first + c, c < ncols (k_cop_normals); streams: device, [K]
void cop_launch_normals(hipStream_t st, uint64_t seed, const uint32_t *streams, int K, int64_t first, int64_t ncols, int antithetic,
                        double *Z, int64_t ldz);
// U[m * ldu + c] = clamp(normcdf(sum_k F[m * K + k] Z[k * ldz + c])), m < M, c < ncols (k_cop_uniforms); all device
void cop_launch_uniforms(hipStream_t st, const double *F, int M, int K, const double *Z, int64_t ldz, int64_t ncols, double *U,
                         int64_t ldu);
// U[(b * set_rows + m) * ldu + c] = clamp(normcdf(shift[b * set_rows + m] + sum_k F[m * K + k] Z[k * ldz + c])), b < B, m < M,
// c < ncols (k_cop_uniforms<true>): the sum as above, then one rounded addition; all device
void cop_launch_uniforms_shifted(hipStream_t st, const double *F, int M, int K, const double *Z, int64_t ldz, int64_t ncols, double *U,
                                 int64_t ldu, const double *shift, int B, int64_t set_rows);

}  // namespace mlmc
