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

// ---- the Student-t copula (copula_t.hip) ----
// what depends on nu alone, made on the host once per call (tcop_constants) and passed to the kernels by value
struct TCopConst {
    double dof, sqrt_dof;
    double A;                          // (nu + 1) / 2
    double c0;                         // Gamma((nu + 1) / 2) / (sqrt(nu pi) Gamma(nu / 2)): the t density at 0
    double t_split;                    // |y| below: the centre series of student_t_cdf, from it on: the tail series
    double a;                          // nu / 2
    double lg_a1;                      // log Gamma(nu / 2 + 1)
};
TCopConst tcop_constants(double dof);
// the degrees of freedom of every entry but one end at 64; the mixing variable of the conditional entry has nu + p, up to 192: the
// capped loops of copula_t.hip stay below half their caps there (tests/conditional_t_cases.py)
constexpr int TCOP_MAX_DOF = 64, TCOP_MAX_DOF_MIX = 192;
// 0, or 1 with the error set: `name` must lie in [1, max_dof] (NaN is outside)
int tcop_check_dof(const char *fn, double dof, int max_dof = TCOP_MAX_DOF, const char *name = "dof");
// s[c] = chi2_mixing_scale(nu, p0 of draw first + c), c < ncols (k_cop_mixing): p0 = uniform j (antithetic: j >> 1) of `stream`
// under `seed`, or with sobol_row (device, [SOBOL_ROW]) the coordinate of point j in that row's dimension
void cop_launch_mixing(hipStream_t st, const TCopConst &C, uint64_t seed, uint32_t stream, const uint64_t *sobol_row, int64_t first,
                       int64_t ncols, int antithetic, double *s);
// s[r * ncols + c] = chi2_mixing_scale(nu, p0 of point j0 + c under seeds[r]), r < R, c < ncols (k_box_mixing), and 1 for a point
// outside [first, first + n): p0 = uniform j of `stream` under seeds[r], or with `table` (device, R tables of table_rows rows) the
// coordinate of point j in row `stream` of seed r's table; seeds: device, [R]
void cop_launch_box_mixing(hipStream_t st, const TCopConst &C, int R, const uint64_t *seeds, uint32_t stream, const uint64_t *table,
                           int table_rows, int64_t j0, int64_t ncols, int64_t first, int64_t n, double *s);
// the lead component of the tl box entries (k_box_lead_weights): w[b] = W0 = T(hi[b][0] / L_00) - T(lo[b][0] / L_00) through the lower
// tail on either side (0 for an empty lead), w[B + b] = the lower end d of the interval of p; L, lo [B][M], hi, w [2 B]: device.
// L_00 of box b is L[b * fstride]: fstride = 0 for one shared factor, the distance of the boxes' factors otherwise (here and below)
void cop_launch_box_lead_weights(hipStream_t st, const TCopConst &C, int M, const double *L, int64_t fstride, const double *lo,
                                 const double *hi, int B, double *w);
// v[(r * B + b) * ncols + c] = the lead score of point j0 + c under seeds[r] in box b, sc[...] = g0[r * ncols + c] (x)
// sqrt((nu + v v) / (nu + 1)) (k_box_lead); v = 0 and sc = 1 for a point outside [first, first + n).  C: the constants of nu; g0: the
// scales of cop_launch_box_mixing with those of nu + 1; `stream` / `table` as there; all device
void cop_launch_box_lead(hipStream_t st, const TCopConst &C, int M, const double *L, int64_t fstride, const double *lo, const double *hi,
                         int B, int R, const uint64_t *seeds, uint32_t stream, const uint64_t *table, int table_rows, int64_t j0, int64_t ncols,
                         int64_t first, int64_t n, const double *g0, const double *w, double *v, double *sc);
// U[m * ldu + c] = (sum_k F[m * K + k] Z[k * ldz + c]) (x) s[c], m < M, c < ncols (k_cop_uniforms, the TSCALE instance): the sum as
// above, then one rounded multiplication; all device
void cop_launch_scaled_product(hipStream_t st, const double *F, int M, int K, const double *Z, int64_t ldz, int64_t ncols, double *U,
                               int64_t ldu, const double *s);
// U[(b * set_rows + m) * ldu + c] = shift[b * set_rows + m] (+) (((sum_k F[m * K + k] Z[k * ldz + c]) (x) s[c]) (x) scale[b]), b < B,
// m < M, c < ncols (k_cop_uniforms, the SHIFT and TSCALE instance): the sum as above, then three rounded operations; all device
void cop_launch_scaled_shifted(hipStream_t st, const double *F, int M, int K, const double *Z, int64_t ldz, int64_t ncols, double *U,
                               int64_t ldu, const double *shift, const double *s, const double *scale, int B, int64_t set_rows);
// U[m * ldu + c] = clamp(student_t_cdf(nu, U[m * ldu + c])) in place, m < M, c < ncols (k_tcop_map)
void cop_launch_t_map(hipStream_t st, const TCopConst &C, int M, int64_t ncols, double *U, int64_t ldu);
// Y[m * ldy + c] = student_t_quantile(nu, clamp(U[m * ldu + c])), NaN for NaN, m < M, c < ncols (k_tcop_scores); all device
void cop_launch_t_scores(hipStream_t st, const TCopConst &C, int M, int64_t ncols, const double *U, int64_t ldu, double *Y, int64_t ldy);

}  // namespace mlmc
