/*
 * mlmc_hip.h -- C ABI of libmlmc_hip.so: MI355X (gfx950) moment estimation and maximum-entropy
 * PDF reconstruction for multilevel Monte Carlo.
 *
 * The reference (GeoMop/MLMC, /root/reference) is pure Python and has no FFI of its own; the
 * boundary it offers for this path is a set of Python call signatures.
 * Each entry point below names the reference interface it replaces (file:line relative to
 * /root/reference).  Host code (the mlmc_amd Python package) binds these with ctypes; INTEGRATION.md shows the
 * stub a maintainer of the reference would add.
 *
 * Conventions: every function returns 0 on success, non-zero on error (message through
 * mlmc_last_error(), thread-local).  The caller owns every buffer passed in; the library owns
 * its device scratch.  `mem_kind` says where a caller buffer lives (host or the bound device).
 * One process binds one device (one process per GPU) and the library works on ONE stream with shared workspaces.
 * Thread safety: every entry point below (all but mlmc_last_error / mlmc_abi_version) takes one library-wide lock, so
 * calls from several host threads are safe and are serialised in arrival order (bindings such as ctypes release the GIL
 * during a call).  Distinct handles may be used from distinct threads concurrently; a multi-call sequence on ONE
 * accumulator (reset ... push ... finalize) belongs to one thread at a time -- the one-call forms mlmc_accum_estimate /
 * mlmc_accum_estimate_packed hold the lock for the whole estimate.
 * All floating point is IEEE fp64, all counts int64.  No CPU fallback exists: without a HIP
 * device every compute entry point fails.
 */
#ifndef MLMC_HIP_H
#define MLMC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLMC_ABI_VERSION 8   /* 2: strides in mlmc_expr_eval, chaining flags, mlmc_accum_estimate_packed; 3: mlmc_wait_event;
                              * 4: x_lo / x_hi in mlmc_basis_desc, mlmc_expr_state, mlmc_accum_kernel_flops;
                              * 5: mlmc_accum_aux_kernel_time; 6: mlmc_linearization_table;
                              * 7: mlmc_maxent_solve_batch, mlmc_density_eval_batch, mlmc_accum_estimate_multi;
                              * 8: mlmc_xcov_create, mlmc_xcov_set_shift; added within 8 (backwards compatible):
                              *    mlmc_percentiles_rows, mlmc_bootstrap_weights, mlmc_bootstrap_create / _destroy / _reset / _accum /
                              *    _finalize / _kernel_time, mlmc_accum_estimate_multi_var, mlmc_density_integrate_batch,
                              *    mlmc_density_cdf_batch, mlmc_density_quantiles_batch,
                              *    mlmc_density_quantiles_kernel_time, mlmc_level_diagnostics, mlmc_diag_merge,
                              *    mlmc_chebyshev_connection_table, mlmc_bootstrap_create_multi, mlmc_bootstrap_finalize_multi,
                              *    mlmc_density_tail_means_batch, mlmc_density_divergences_batch, mlmc_density_moments_batch,
                              *    mlmc_density_sample_batch, mlmc_density_sample_joint_batch, mlmc_density_scores_batch,
                              *    mlmc_density_sample_conditional_batch, mlmc_sobol_table (and the flag MLMC_SAMPLE_SOBOL of the
                              *    three sampling entries), mlmc_copula_box_prob_batch, mlmc_copula_box_draws_batch,
                              *    mlmc_bootstrap_create_xcov, mlmc_bootstrap_set_shift, mlmc_bootstrap_finalize_xcov,
                              *    mlmc_scenario_aggregates, mlmc_rows_weighted_sums, mlmc_concordance_counts,
                              *    mlmc_student_t_cdf, mlmc_chi2_mixing_scale, mlmc_density_sample_joint_t_batch,
                              *    mlmc_copula_box_prob_t_batch, mlmc_copula_box_draws_t_batch,
                              *    mlmc_density_sample_conditional_t_batch, mlmc_chi2_conditional_scale,
                              *    mlmc_student_t_quantile, mlmc_copula_log_density,
                              *    mlmc_copula_box_prob_tc_batch, mlmc_copula_box_draws_tc_batch,
                              *    mlmc_copula_box_prob_tl_batch, mlmc_copula_box_draws_tl_batch,
                              *    mlmc_copula_box_prob_pf_batch, mlmc_copula_box_prob_t_pf_batch,
                              *    mlmc_copula_box_prob_tl_pf_batch, mlmc_copula_box_order_batch */

/* basis kinds -- mlmc/moments.py: Legendre :174-229, Monomial :111-130, Fourier :133-171;
 * IDENTITY = the quantity itself (estimate_mean of a plain quantity, quantity_estimate.py:22-80);
 * SPLINE = cubic B-spline moments.  The reference imports scipy's BSpline (moments.py:3) but defines no spline class
 * (SURVEY fact 2): phi_0 = 1, phi_r = B_r (r = 1..size-1) of the clamped uniform cubic B-spline basis B_0..B_{size-1}
 * on ref_domain, pinned against scipy.interpolate.BSpline ("parity unpinned" with respect to the reference). */
enum { MLMC_LEGENDRE = 0, MLMC_MONOMIAL = 1, MLMC_FOURIER = 2, MLMC_IDENTITY = 3, MLMC_SPLINE = 4 };
/* accumulation modes */
enum {
    MLMC_MODE_MOMENTS = 0,  /* qe.moments + estimate_mean    (quantity_estimate.py:96-119, :22-80)  K = R      */
    MLMC_MODE_COV = 1       /* qe.covariance + estimate_mean (quantity_estimate.py:122-156, :22-80) K = R * R  */
};
enum { MLMC_HOST = 0, MLMC_DEVICE = 1 };

typedef struct mlmc_basis mlmc_basis;
typedef struct mlmc_accum mlmc_accum;

/* Plain-data image of a reference Moments object (mlmc/moments.py:10-39):
 * t = (x - shift) * scale + ref0 (after log(x) if is_log); values with t outside [ref0, ref1]
 * are NaN-masked when is_clip (Moments.clip, moments.py:58-67).  `matrix` (row-major
 * [out_size][size], host pointer, may be NULL) is TransformedMoments._transform (moments.py:232-259).
 * x_lo / x_hi (used when is_log and is_clip): the keep / drop decision of a sample under log=True is taken on the RAW
 * value, keep <=> x_lo <= x <= x_hi, where x_lo is the smallest and x_hi the largest double whose
 * t = (log(x) - shift) * scale + ref0, computed with the CALLER's log, lies in [ref0, ref1].  The map x -> t is monotone,
 * so the caller finds both by bisection over the doubles (<= 64 steps each); sample counts are then bit-identical to the
 * caller's own NumPy / libm path, whatever the last bit of the device's log is (moments.py:27-39,58-73 use np.log).
 * x_lo == x_hi == 0 asks the library to bisect with the C library's log() of the host. */
typedef struct {
    int32_t kind;
    int32_t size;       /* number of basis functions R of the underlying family */
    double shift;       /* Moments._linear_shift */
    double scale;       /* Moments._linear_scale */
    double ref0, ref1;  /* Moments.ref_domain */
    int32_t is_log;     /* Moments._is_log */
    int32_t is_clip;    /* Moments._is_clip (safe_eval) */
    int32_t out_size;   /* rows of `matrix`; 0 = no linear transform */
    int32_t reserved;
    const double *matrix;
    double x_lo, x_hi;  /* raw-value keep interval under is_log && is_clip (see above) */
} mlmc_basis_desc;

/* ---- runtime -------------------------------------------------------------------------- */
/* Bind this process to HIP device `device` (>= 0). flags: bit0 = record HIP-event timing of the
 * accumulation kernels (read back with mlmc_accum_kernel_time). */
int mlmc_init(int device, int flags);
void mlmc_shutdown(void);
/* Run all later work on the caller's HIP stream (e.g. the stream RCCL collectives are enqueued on), so that
 * mlmc_accum_finalize_packed(..., MLMC_DEVICE) followed by an all-reduce needs no host synchronisation in between. */
int mlmc_set_stream(void *hip_stream);
/* Make the library's stream wait for a HIP event recorded on another stream of the same device (asynchronous for the
 * host): the feed of a storage that arrives in many chunks (SampleStorageHDF: one `collected_values[chunk_slice]` read per
 * chunk, mlmc/tool/hdf5.py:353-376) copies chunk k + 1 from pinned host memory on a copy stream while the kernels of chunk k
 * run here; every later launch of the library is ordered behind the event. */
int mlmc_wait_event(void *hip_event);
/* Wait until everything the library has enqueued on its stream is done (asynchronous entry points: mlmc_accum_push
 * with device buffers, mlmc_expr_eval, mlmc_accum_finalize_packed(MLMC_DEVICE)). */
int mlmc_synchronize(void);
const char *mlmc_last_error(void);
int mlmc_abi_version(void);
/* name[<=256], CU count, wavefront size, total HBM bytes of the bound device */
int mlmc_device_info(char *name, int name_len, int *n_cu, int *wave_size, int64_t *hbm_bytes);

/* ---- moment functions ----------------------------------------------------------------- */
int mlmc_basis_create(const mlmc_basis_desc *desc, mlmc_basis **out);
void mlmc_basis_destroy(mlmc_basis *b);
/* Moments.eval_all(value, size) (moments.py:90-93; legvander/polyvander/Fourier/TransformedMoments
 * ._eval_all :122-126,:145-162,:195-197,:256-259): out[i * size + r] for i < n, r < size.
 * Masked values give NaN in every column, as in the reference. */
int mlmc_basis_eval(const mlmc_basis *b, const double *x, int64_t n, int32_t size, double *out, int mem_kind);

/* ---- level-difference accumulation (the hot loop) ------------------------------------- */
/* One accumulator = one estimate_mean() call (quantity_estimate.py:22-80) over `n_levels` levels of a
 * quantity with `n_comp` (= M) scalar components; rows K = n_comp * R (MOMENTS) or n_comp * R * R (COV),
 * row index m * R + r / m * R * R + i * R + j (mom_at_bottom / cov_at_bottom = True layout). */
/* mode may carry MLMC_MODE_MEAN_ONLY: the caller will read only the sums s (level means), so the passes that exist
 * solely for sp are skipped -- the covariance accumulates one Gram matrix (D^T S) instead of three, TransformedMoments
 * skip their diff-Gram pass; the skipped sp come back as NaN.  (Estimate.construct_density, estimator.py:304-331, uses
 * only the means of both of its estimates.) */
#define MLMC_MODE_MEAN_ONLY 0x100
int mlmc_accum_create(const mlmc_basis *b, int32_t n_levels, int32_t mode, int32_t n_comp, mlmc_accum **out);
void mlmc_accum_destroy(mlmc_accum *a);
int mlmc_accum_reset(mlmc_accum *a);
/* One chunk of level `level`: fine[m * n + k], coarse[m * n + k] (coarse == NULL at level 0:
 * SampleStorage.sample_pairs_level returns [M, n, 1] there, sample_storage.py:261-285).
 * Replaces eval_moments/eval_cov + mask_nan_samples + the two np.sum of quantity_estimate.py:43-65.
 * Asynchronous on the library's stream.  Host buffers are staged before the call returns; DEVICE buffers must stay
 * valid until the next mlmc_accum_finalize / mlmc_accum_reset: chunks of different levels are gathered and processed
 * by ONE kernel launch (one grid for a whole multi-level estimate). */
int mlmc_accum_push(mlmc_accum *a, int32_t level, const double *fine, const double *coarse, int64_t n, int mem_kind);
/* Writes per level l: n[l] (kept samples), n_rm[l] (NaN-masked samples), s[l * K + k] = sum of
 * level differences, sp[l * K + k] = sum of squared differences (quantity_estimate.py:46-47,64-65).
 * Outputs in host or device memory (device: for an RCCL all-reduce over ranks before the host reads them).
 * Synchronises the stream; idempotent. */
int mlmc_accum_finalize(mlmc_accum *a, int64_t *n, int64_t *n_rm, double *s, double *sp, int mem_kind);
/* reset + push of n_chunks chunks + finalize in one call (one host round trip per estimate): chunk k is
 * (levels[k], fine[k], coarse[k] or NULL, n[k]); all chunk buffers of one kind (mem_kind).  Results as mlmc_accum_finalize
 * with MLMC_HOST outputs. */
int mlmc_accum_estimate(mlmc_accum *a, int32_t n_chunks, const int32_t *levels, const double *const *fine,
                        const double *const *coarse, const int64_t *n_samples, int mem_kind, int64_t *n, int64_t *n_rm,
                        double *s, double *sp);
/* The same with the results as mlmc_accum_finalize_packed leaves them (one fp64 buffer n | n_rm | s | sp in host or
 * device memory): the rank-local half of a multi-GPU estimate, stream-ordered before the all-reduce when device. */
int mlmc_accum_estimate_packed(mlmc_accum *a, int32_t n_chunks, const int32_t *levels, const double *const *fine,
                               const double *const *coarse, const int64_t *n_samples, int mem_kind, double *packed,
                               int packed_kind);
/* Same results in ONE fp64 buffer [n(L) | n_rm(L) | s(L*K) | sp(L*K)] (counts as exact doubles): a single packed
 * all-reduce (RCCL) then carries everything a multi-GPU estimate has to exchange.  With MLMC_DEVICE the call is
 * asynchronous (stream-ordered); with MLMC_HOST it synchronises. */
int mlmc_accum_finalize_packed(mlmc_accum *a, double *packed, int mem_kind);
/* HIP-event time (ms) and launch count of the dominant accumulation kernel since create or since the previous
 * call of this function (it returns the totals and clears them; mlmc_accum_reset leaves them alone; needs
 * mlmc_init flag bit0); also the algorithmic HBM bytes those launches had to read.  Waits for the last launch. */
int mlmc_accum_kernel_time(mlmc_accum *a, double *ms, int64_t *launches, int64_t *alg_bytes);
/* Matrix-core flops the covariance launches counted by mlmc_accum_kernel_time have EXECUTED since create or since the
 * previous call of this function: one v_mfma_f64_16x16x4_f64 is 2 * 16 * 16 * 4 flops and covers four samples, i.e. 512
 * flops per 16 x 16 output tile and sample, times the tiles the kernels' tile lists name.  Symmetric Gram tiles are computed
 * once (R = 64, pair level, mean + variance: 16 + 16 + 10 = 42 tiles instead of 48), so the figure is BELOW the reference-
 * form count 6 R^2 per pair (quantity_estimate.py:131-147); it is the numerator of a physical matrix-pipe fraction.
 * Returns the total and clears it. */
int mlmc_accum_kernel_flops(mlmc_accum *a, int64_t *mfma_flops);
/* A MLMC_MODE_COV accumulator WITH variances of 17..128 plain Legendre or monomial moments splits the work of its large chunks
 * (>= 10^5 samples at 33..128 moments, >= 1.5 x 10^6 at 17..32; MLMC_HIP_LINEARIZE_MIN_N overrides; smaller chunks keep all
 * three Gram matrices, the level sums are additive): the matrix cores
 * accumulate only the two Gram matrices of the VARIANCE (G1, G2: 26 instead of 42 tiles per pair at R = 64), and the MEAN
 * (quantity_estimate.py:131-147 + :59-65: level sums of f_i f_j - c_i c_j) comes from the level sums of the 2 R - 1 moments
 * of the same family through the product linearisation phi_i phi_j = sum_k c_ijk phi_k (Legendre: Adams' formula, non-negative
 * coefficients that sum to one) -- one mean-only pass of the moments kernel over the same chunks with the same keep / drop
 * decisions, contracted on the device at finalize.  Same outputs, same counts; the means agree with the direct sums to rounding
 * (a convex combination of sums instead of sums of products).  A large chunk WITHOUT coarse values (level 0) of <= 64 such
 * moments needs no matrix pass at all: with one value per sample the second moments linearise too, (phi_i phi_j)^2 =
 * sum_k c2_ijk phi_k with k < 4 R - 3, so the level sums of 4 R - 3 moments (two windows of the same mean-only kernel, which
 * then also does the counting) give both sum f_i f_j and sum (f_i f_j)^2; MLMC_HIP_LINEARIZE_LEVEL0=0 keeps level 0 on the matrix
 * cores.  MLMC_HIP_LINEARIZE=0 in the environment keeps all three Gram matrices of every chunk on the matrix cores.  This call
 * reports the HIP-event time, launches and algorithmic bytes of the auxiliary moments passes (zeros when the accumulator has
 * none), like mlmc_accum_kernel_time does for the matrix-core launches. */
int mlmc_accum_aux_kernel_time(mlmc_accum *a, double *ms, int64_t *launches, int64_t *alg_bytes);
/* The coefficient tables of those linearisations, as the accumulators use them (host arithmetic only: needs no device, e.g.
 * for checking them against exact rational values): squares == 0: phi_i phi_j = sum_k c_ijk phi_k, K = 2 R - 1;
 * squares != 0: (phi_i phi_j)^2 = sum_k c2_ijk phi_k, K = 4 R - 3.  out [K][R * R] (k-major), out_len >= K * R * R.
 * kind: MLMC_LEGENDRE or MLMC_MONOMIAL, 1 <= R <= 128 (squares: R <= 64).
 * squares == 2 / 3 (MLMC_LEGENDRE only): the same two tables for level sums of CHEBYSHEV polynomials T_m of the transformed
 * value, which the inner accumulators of a Legendre covariance sum where they have more than 64 terms (one FMA per term):
 * phi_i phi_j = sum_m c'_ijm T_m, (phi_i phi_j)^2 = sum_m c2'_ijm T_m, with c'_ijm = sum_k c_ijk a_km and the exact connection
 * P_k = sum_m a_km T_m folded in on the host in extended precision.  Same shapes and limits as 0 / 1; other values fail. */
int mlmc_linearization_table(int32_t kind, int32_t R, int32_t squares, double *out, int64_t out_len);

/* The connection from Legendre to Chebyshev polynomials, T_m = sum_{k <= m} b_mk P_k for m, k < M <= 64: out[m * M + k], host
 * arithmetic in extended precision, rounded once (no device needed).  b_00 = 1, b_0k = 0, b_mk = 0 unless k = m (mod 2), every row
 * sums to one.  A covariance with variances of 49..64 Legendre moments takes the first 64 Chebyshev level sums of its pair levels from
 * the Legendre difference sums its matrix kernel accumulates on the side (MLMC_HIP_LINEARIZE_ROWSUMS=0: from a full auxiliary pass). */
int mlmc_chebyshev_connection_table(int32_t M, double *out, int64_t out_len);

/* Mean-only level sums of a quantity of M components, each with ITS OWN moment functions (Estimate.construct_densities:
 * construct_density of every scalar component, estimator.py:304-331): bases[m] (m < M) are plain Legendre, monomial or Fourier
 * members of ONE family with size >= K, each with its own domain, log, x_lo / x_hi and safe_eval; component m of chunk c is row
 * m of fine[c] / coarse[c] ([M][n] DEVICE buffers, coarse[c] NULL at level 0).  Each component is masked on its own, by the rule
 * mlmc_accum_push applies to a one-component chunk (the fine AND the coarse value kept by the domain transform, no NaN), so
 * n / n_rm are bit-identical to M scalar estimates.  One pass per chunk for all components (one launch per chunk, plus a
 * fixed-order merge).  Outputs (host): n[l * M + m], n_rm[l * M + m], sums[(l * M + m) * K + k] = level sums of the
 * differences phi_k(fine) - phi_k(coarse) of component m.  Synchronises. */
int mlmc_accum_estimate_multi(int32_t M, const mlmc_basis *const *bases, int32_t K, int32_t n_levels, int32_t n_chunks,
                              const int32_t *levels, const double *const *fine, const double *const *coarse,
                              const int64_t *n_samples, int64_t *n, int64_t *n_rm, double *sums);
/* The same pass with the level variances (Estimate.estimate_component_moments / _diff_vars / _diff_vars_regression: the scalar
 * estimate_moments / estimate_diff_vars of every component, estimator.py:32-93) -- added within 8.  Arguments, argument checks,
 * masking rule and errors are those of mlmc_accum_estimate_multi (messages name this entry and the component); in addition
 * sums_sq[(l * M + m) * K + k] = level sums of (phi_k(fine) - phi_k(coarse))^2 of component m.  Both sums of a (sample block,
 * component, term window) stay in registers and are merged in a fixed order: the same chunks in the same order give the same
 * bits.  Device scratch stays within 64 MiB (components run in groups when L * M * K exceeds about 3.5 M).  Synchronises once. */
int mlmc_accum_estimate_multi_var(int32_t M, const mlmc_basis *const *bases, int32_t K, int32_t n_levels, int32_t n_chunks,
                                  const int32_t *levels, const double *const *fine, const double *const *coarse,
                                  const int64_t *n_samples, int64_t *n, int64_t *n_rm, double *sums, double *sums_sq);

/* ---- per-level convergence diagnostics of every component (level_diag.hip) -- added within 8 ----------------------------
 * The statistics of the standard MLMC convergence tests (Giles' mlmc_test), per level l and component m.  A sample is kept when
 * neither its fine nor (in a level with coarse samples) its coarse value is NaN -- each component on its own; +-inf is a value
 * like any other.  With y = fl(f - c) (without coarse samples: y = f), M_k(x) = sum (x - mean x)^k over the kept samples and
 * C_fc = sum (f - mean f)(c - mean c), the MLMC_DIAG_NSTAT statistics are, in this order,
 *     mean_y, M2_y, M3_y, M4_y, mean_f, M2_f, mean_c, M2_c, C_fc
 * Without coarse samples the last three are NaN; without a kept sample all nine are NaN; one kept sample gives the means as
 * the values and every M as 0.
 * A kept +-inf makes the means it enters +-inf (NaN where both signs, or inf - inf in y, meet), as estimate_mean gives them, and
 * the central sums it enters NaN; the counts are not affected.
 * Arguments and argument checks are those of mlmc_accum_estimate_multi_var without the bases ([M][n] DEVICE rows per chunk),
 * except that M >= 1 is required; messages name this entry.  coarse[c] is NULL for a chunk without coarse samples and is not
 * read at level 0; a level (above 0) whose non-empty chunks mix NULL and non-NULL coarse is an error.
 * Outputs (host): n[l * M + m], n_rm[l * M + m], stats[(l * M + m) * MLMC_DIAG_NSTAT + s].  Two passes per chunk (means, then
 * sums about them with the exact correction for the means' rounding: no cancellation at any offset of the data), fixed-order
 * reductions, no floating-point atomics; the samples per workgroup depend on n alone, so a component's bits depend neither on
 * M nor on its row, and the same chunks in the same order give the same bits.  The chunks of a level are merged in the order
 * of the call with the arithmetic of mlmc_diag_merge.  Device scratch stays within 64 MiB plus 88 bytes per (chunk,
 * component).  Synchronises once. */
#define MLMC_DIAG_NSTAT 9
int mlmc_level_diagnostics(int32_t M, int32_t n_levels, int32_t n_chunks, const int32_t *levels, const double *const *fine,
                           const double *const *coarse, const int64_t *n_samples, int64_t *n, int64_t *n_rm, double *stats);
/* The nine statistics of the union of two disjoint sample sets, a of na and b of nb samples, by the pairwise update formulas of
 * Chan, Golub and LeVeque (mean, M2) and Pebay (M3, M4, co-moment).  Host arithmetic only: needs no device.  An empty side
 * (count 0) returns the other side unchanged, bit for bit.  out may be a or b. */
int mlmc_diag_merge(const double *a, int64_t na, const double *b, int64_t nb, double *out);

/* ---- covariance between the components of a vector quantity ---------------------------------------------------------
 * An accumulator of the M x M level sums, per level l and kept sample k,
 *     Y_k = (f_k - a)(f_k - a)^T - (c_k - a)(c_k - a)^T      (no coarse values -- level 0: Y_k = (f_k - a)(f_k - a)^T)
 *     s[l] = sum_k Y_k,   sp[l] = sum_k Y_k o Y_k            (element-wise square)
 * f_k / c_k: the M fine / coarse component values of sample k, a: the shift (the same for every level, fine and coarse).  A
 * sample is dropped from the whole matrix if any of its M fine or M coarse values is NaN (quantity_estimate.py:6-14, over the
 * [M, n, 2] chunk).  With a = 0, entry (i, j) is the reference's estimate_mean(q_i * q_j).  Both sums are bitwise symmetric.
 * The result is an ordinary accumulator: mlmc_accum_push (chunks [M][n], component-major, coarse NULL at level 0), reset,
 * finalize, estimate, estimate_packed, finalize_packed, kernel_time (the mask pass, the matrix-core launch and the reduction of
 * every chunk), kernel_flops (executed v_mfma_f64_16x16x4_f64 flops) and destroy work on it; K = M * M, row i * M + j.
 * M: 1 .. 1024.  flags: 0 or MLMC_MODE_MEAN_ONLY (sp comes back as NaN).  Deterministic: the same chunks pushed in the same
 * order give the same bits. */
int mlmc_xcov_create(int32_t M, int32_t n_levels, int32_t flags, mlmc_accum **out);
/* The shift a (host array of M doubles, finite; NULL = zeros).  It takes effect at the next mlmc_accum_reset (mlmc_accum_estimate
 * and mlmc_accum_estimate_packed reset first); an error while pushes since the last reset are pending. */
int mlmc_xcov_set_shift(mlmc_accum *a, const double *shift_host);

/* ---- maximum-entropy density (mlmc/tool/simple_distribution.py:9-327) ------------------ */
typedef struct {
    double tol;          /* gradient-norm tolerance (estimate_density_minimize tol, :50) */
    int32_t max_it;      /* Newton iterations (reference: trust-ncg maxiter 20, :60) */
    int32_t n_intervals; /* composite Gauss-Legendre sub-intervals on [a, b] (0 = default 64) */
    int32_t gauss_degree;/* points per sub-interval (reference uses 21, :45); 0 = 21 */
    int32_t reserved;
    double stab_penalty; /* Distribution._stab_penalty (distribution.py:236); 0 for SimpleDistribution */
    double penalty_coef; /* end-point decay penalty coefficient (distribution.py:47 = 10; simple: 0) */
    int32_t decay_left, decay_right; /* force_decay flags */
} mlmc_maxent_opts;

typedef struct {
    int32_t nit;
    int32_t success;
    double fun;        /* final functional value */
    double grad_norm;  /* ||gradient||_2 at the solution (result.fun_norm, :93) */
    double moment0;    /* integral of the density before the normalisation fix (:81-86) */
    int32_t n_quad;
    int32_t reserved;
} mlmc_maxent_info;

/* Minimise F(l) = sum_i mu_i l_i / sigma_i + int exp(-phi(x).l/sigma) dx (simple_distribution.py:259-327)
 * starting from lambda_io (size R1 = number of moments used, <= basis out size); on return lambda_io holds
 * the multipliers (normalisation fix of :86 NOT applied; see moment0), grad_out / hess_out (may be NULL) the final
 * gradient [R1] and Hessian [R1 * R1].  prev_lambda/n_prev: Distribution's stabilisation term (distribution.py:358-359), may be NULL/0.
 * On EVERY exit (converged, iteration cap, regularisation limit) grad_out, hess_out, info->fun, info->grad_norm and
 * info->moment0 are values AT THE RETURNED lambda_io, on the rule of n_intervals x gauss_degree points; without penalties
 * hess_out is symmetric bit for bit.  success = 1 <=> grad_norm < tol. */
int mlmc_maxent_solve(const mlmc_basis *b, const double *mu, const double *sigma, int32_t R1, double a, double bnd_b,
                      const mlmc_maxent_opts *opts, const double *prev_lambda, int32_t n_prev, double *lambda_io,
                      double *grad_out, double *hess_out, mlmc_maxent_info *info);
/* SimpleDistribution.density (:96-105): out[i] = exp(clip(-phi(x_i).lambda/sigma, -200, 200)) */
int mlmc_density_eval(const mlmc_basis *b, const double *lambda, const double *sigma, int32_t R1, const double *x,
                      int64_t n, double *out, int mem_kind);
/* integral of the density over [lo_i, hi_i] by `degree`-point Gauss-Legendre per interval (cdf :108-125) */
int mlmc_density_integrate(const mlmc_basis *b, const double *lambda, const double *sigma, int32_t R1, const double *lo,
                           const double *hi, int64_t n, int32_t degree, double *out);
/* B independent problems of mlmc_maxent_solve's functional WITHOUT penalties (SimpleDistribution.estimate_density_minimize,
 * one per scalar component of a vector quantity) in one launch: one workgroup owns one problem for the whole solve, so B may
 * exceed the CU count and a problem's result is bit for bit the same alone, anywhere in any batch.  Problem i: basis bases[i]
 * (its own transform and domain), R1[i] <= 128 moments, domain [a[i], b[i]].  mu, sigma, lambda_io, grad_out are [B][R1max],
 * hess_out [B][R1max][R1max] (R1max = max R1[i]; entries beyond a problem's R1 are zero in the outputs, lambda_io keeps them);
 * grad_out / hess_out may be NULL; info [B].  One opts for the batch (same quadrature for every problem); opts carrying
 * stab_penalty or penalty_coef are rejected (the penalised Distribution stays on mlmc_maxent_solve).  Argument errors name the
 * problem index; a problem that does not converge is no error (info[i].success = 0).  B = 0 is a no-op.  Same algorithm,
 * constants and result fields as mlmc_maxent_solve. */
int mlmc_maxent_solve_batch(int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *a, const double *b,
                            const double *mu, const double *sigma, const mlmc_maxent_opts *opts, double *lambda_io,
                            double *grad_out, double *hess_out, mlmc_maxent_info *info);
/* mlmc_density_eval of B problems in one launch: lambda / sigma [B][R1max]; x / out host arrays holding the problems' points one
 * after another (problem i: n[i] points at offset n[0] + ... + n[i - 1]).  Each value is bit for bit mlmc_density_eval's. */
int mlmc_density_eval_batch(int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda, const double *sigma,
                            const double *x, const int64_t *n, double *out);
/* mlmc_density_integrate of B problems in one launch: lambda / sigma [B][R1max]; lo / hi / out host arrays holding the problems'
 * intervals one after another (problem i: n[i] intervals).  Each value is bit for bit mlmc_density_integrate's.  Argument errors
 * name the problem index; B = 0 and n[i] = 0 are no-ops. */
int mlmc_density_integrate_batch(int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                                 const double *sigma, const double *lo, const double *hi, const int64_t *n, int32_t degree,
                                 double *out);
/* CDF on the solver's rule, and its inverse, of B problems in one call.  For problem i with domain [a[i], b[i]] and the rule
 * (n_intervals, gauss_degree; 0 = the solver's defaults 64 and 21) let e_j = a + j h (fp64, h = (b - a) / n_intervals, e_n = b)
 * be the cell edges, C_j the gauss_degree-point Gauss-Legendre integral of the density over cell j (the arithmetic of
 * mlmc_density_integrate), P_0 = 0, P_{j+1} = P_j + C_j in cell order and T = P_n the mass.  Then
 *     Fhat(x) = (P_j + I(e_j, x)) / T for x in cell j (I: the same rule on the partial cell), 0 for x <= a, 1 for x >= b, NaN for NaN,
 * is what mlmc_density_cdf_batch evaluates at x, and mlmc_density_quantiles_batch returns Q(p) = the x in [a, b] with
 * Fhat(x) = p: Q(0) = a and Q(1) = b exactly, NaN for p outside [0, 1] or NaN.  Layout as mlmc_density_eval_batch: lambda / sigma
 * [B][R1max], the problems' points one after another with counts n[i] (host, int64); a, b [B] host; mass_out [B] host (may be
 * NULL) receives T; mem_kind (MLMC_HOST / MLMC_DEVICE) applies to x / p and out.  One thread owns one point and every sum has
 * a fixed order: a value does not depend on the batch, on the problem's position in it or on the other points.  Argument errors
 * of one problem name its index (null basis, R1 out of range, a >= b or non-finite, n < 0, unsupported basis kind = IDENTITY);
 * errors of the call as a whole name none (a null array, B < 0, gauss_degree outside 0..64, n_intervals < 0, bad mem_kind); B = 0 and n[i] = 0 are no-ops; a problem whose mass is not finite and positive gives NaN for
 * all its points and is no error. */
int mlmc_density_cdf_batch(int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda, const double *sigma,
                           const double *a, const double *b, int32_t n_intervals, int32_t gauss_degree, const double *x,
                           const int64_t *n, double *out, double *mass_out, int mem_kind);
int mlmc_density_quantiles_batch(int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                                 const double *sigma, const double *a, const double *b, int32_t n_intervals, int32_t gauss_degree,
                                 const double *p, const int64_t *n, double *out, double *mass_out, int mem_kind);
/* Tail means (expected shortfall, CVaR) of B problems in one call -- added within 8.  Edges e_j, cell integrals C_j, prefix P and
 * mass T = P_n are those of mlmc_density_cdf_batch, bit for bit the table of the quantile entry.  On the nodes t_k and weights
 * w_k of C_j let
 *     A_j = sum_k w_k (t_k - a) rho(t_k),   B_j = sum_k w_k (b - t_k) rho(t_k)
 * (the anchors are the domain ends in full and partial cells alike: every term is non-negative and nothing cancels, whatever the
 * sign of the domain), V_0 = 0, V_{j+1} = V_j + A_j in cell order, S_n = W_n = 0, S_j = S_{j+1} + C_j, W_j = W_{j+1} + B_j from the
 * last cell down.  For x in [a, b], j the largest index below n with e_j <= x and I, A(.,.), B(.,.) the same rule on a partial cell,
 *     m_lo(x) = P_j + I(e_j, x)           lower(x) = a + (V_j + A(e_j, x)) / m_lo(x)            = E[X | X <= x]
 *     m_hi(x) = S_{j+1} + I(x, e_{j+1})   upper(x) = b - (W_{j+1} + B(x, e_{j+1})) / m_hi(x)    = E[X | X >= x]
 * and a tail without mass (m_lo == 0 or m_hi == 0) returns x itself, so lower(a) = a and upper(b) = b.  For every probability p the
 * entry writes q_out = Q(p), bit for bit the value of mlmc_density_quantiles_batch for the same problem and p, lower_out =
 * lower(Q(p)) (the lower expected shortfall at level p) and upper_out = upper(Q(p)) (the upper one).  All three are NaN for p
 * outside [0, 1] or NaN, and for every point of a problem whose mass T is not finite and positive (no error).  mean_out [B] host
 * (may be NULL) receives a + V_n / T, mass_out [B] host (may be NULL) T.  p lower + (1 - p) upper = mean holds only up to the
 * resolution of the rule: the two partial-cell rules of a point do not add up to the cell's rule exactly.  Layout, conventions,
 * argument errors and no-ops as mlmc_density_quantiles_batch; mem_kind applies to p, q_out, lower_out and upper_out.  One thread
 * owns one point and every sum has a fixed order: a value does not depend on the batch, on the problem's position in it or on the
 * other points.  One host wait. */
int mlmc_density_tail_means_batch(int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                                  const double *sigma, const double *a, const double *b, int32_t n_intervals,
                                  int32_t gauss_degree, const double *p, const int64_t *n, double *q_out, double *lower_out,
                                  double *upper_out, double *mass_out, double *mean_out, int mem_kind);
/* Divergences between pairs of the B problems in one call -- added within 8.  Problems as in mlmc_density_cdf_batch (basis, R1,
 * lambda, sigma, domain [a[i], b[i]]).  Pair k compares problem first[k], the prior p, with problem second[k], the posterior q (the
 * roles of KL_divergence(prior_density, posterior_density, a, b), simple_distribution.py:443-464) on [lo[k], hi[k]]; a problem may
 * appear in any number of pairs.  lo == hi == NULL: the intersection [max(a_p, a_q), min(b_p, b_q)] of the two domains.  The rule
 * (n_intervals, gauss_degree; 0 = 64 and 21) has the cell edges e_j = lo + j h (fp64, h = (hi - lo) / n_intervals, e_n = hi) and
 * on every cell the nodes t and weights w of mlmc_density_integrate.  At a node let e_p, e_q be the clipped exponents
 * clip(-sum_r c_r Q_r(t), +-200) of the two problems, rho_p = exp(e_p), rho_q = exp(e_q) (bit for bit the values of
 * mlmc_density_eval), d = e_q - e_p, x = expm1(d), y = expm1(d / 2).  out[k][c] is the rule's sum of the integrand of column c: */
enum {
    MLMC_DIV_KL = 0,     /* rho_p (x - d)            int p log(p / q) - p + q: the positivity-preserving form, no log, no division */
    MLMC_DIV_L2SQ = 1,   /* (rho_p rho_p) (x x)      int (q - p)^2 */
    MLMC_DIV_TV = 2,     /* (rho_p / 2) |x|          1/2 int |q - p| */
    MLMC_DIV_H2 = 3,     /* (rho_p / 2) (y y)        1/2 int (sqrt q - sqrt p)^2 */
    MLMC_DIV_MASS_P = 4, /* rho_p                    mass of p on the interval */
    MLMC_DIV_MASS_Q = 5, /* rho_q                    mass of q on the interval */
    MLMC_DIV_COUNT = 6
};
/* The densities enter as they are, without normalisation; the two masses let the caller normalise.  Every integrand is formed
 * from rho_p and d, so a pair of a problem with itself gives exactly 0 in the first four columns and equal masses.  Order of the
 * sums: per cell one FMA per node in node order, then times half the cell width (the arithmetic of mlmc_density_integrate); the
 * cells are added in cell order.  Hence with [lo, hi] = [a, b] of the prior MASS_P is bit for bit the mass_out of
 * mlmc_density_cdf_batch for that problem and rule, and a pair's values depend neither on the batch nor on the pair's position
 * nor on how often its problems are used.  A node outside the domain of either basis (density NaN), or NaN multipliers, make
 * all six values of the pair NaN and are no error; oppositely clipped exponents (d > 354.89) overflow x x, and with it L2SQ, to
 * inf, which is no error either.  first / second [P] host int32, lo / hi [P] host (both or neither NULL), out [P][6] host.  Errors
 * of one problem name the problem as in mlmc_density_cdf_batch; errors of one pair name the pair (an index outside 0..B-1, lo or
 * hi not finite or lo >= hi, an interval not inside both domains, an empty intersection); errors of the call as a whole name
 * nothing.  B = 0 or P = 0 is a no-op.  One workgroup per pair, no atomics; one host wait. */
int mlmc_density_divergences_batch(int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                                   const double *sigma, const double *a, const double *b, int32_t n_intervals,
                                   int32_t gauss_degree, int64_t P, const int32_t *first, const int32_t *second, const double *lo,
                                   const double *hi, double *out);
/* Expectations under the densities of B problems in one call -- added within 8: moments in a basis of the caller's choice, mass
 * and entropy.  Problems and rule as in mlmc_density_cdf_batch (basis, R1, lambda / sigma [B][R1max], domain [a[i], b[i]],
 * n_intervals, gauss_degree; 0 = 64 and 21).  Problem i has in addition a test basis test[i] of any of the four kinds, plain or
 * with a matrix, with its own domain, transform, log and clip flags (unrelated to the density's basis), and a count K[i] of its
 * outputs, 1 <= K[i] <= out_size (size for a plain basis).  Its underlying terms are S = size if it has a matrix, else K[i];
 * S <= 512.  The rule: edges e_j = a + j h (fp64, h = (b - a) / n_intervals, e_n = b), per cell half = (e_{j+1} - e_j) / 2,
 * mid = (e_{j+1} + e_j) / 2, nodes t_k = fma(half, g_k, mid) and weights w_k of mlmc_density_integrate.  At a node rho = exp(e)
 * and the clipped exponent e = clip(-sum_r c_r Q_r(t), +-200) are those of mlmc_density_eval (bit for bit), and q_r(t), r < S,
 * are the underlying terms of the test basis at its own transform of t (Legendre: the scaled monic polynomials, P_r = c_r q_r).
 * For every column f in {q_0 .. q_{S-1}, 1, -e}
 *     C_j[f] = (sum over k in node order of acc = fma(w_k, rho f, acc)) * half,     s[f] = sum over j in cell order of C_j[f],
 * then on the host m_r = c_r s[q_r] and, for a basis with a matrix, psi_j = sum_r matrix[j][r] m_r in r order in plain fp64.
 * out [B][Kmax] host, Kmax = max K[i]: the K[i] raw moments int psi_j rho of the density as it is (not normalised), zeros beyond
 * K[i].  mass_out [B] host (may be NULL): the column 1, bit for bit the mass_out of mlmc_density_cdf_batch for the problem and
 * rule.  entropy_out [B] host (may be NULL): the column -e, -int rho log rho with the clipped exponent; the differential entropy
 * of the normalised density is entropy / T + log T.  A node where the density is outside its basis' domain, or NaN multipliers,
 * make every output of the problem NaN; a node the test basis does not keep makes the problem's moments NaN and leaves mass and
 * entropy alone; neither is an error.  Argument errors and no-ops as mlmc_density_cdf_batch; a null test basis, an IDENTITY test
 * basis, K[i] out of range or S > 512 is an error that names the problem.  A problem's values depend neither on the batch nor on
 * its position in it nor on the other problems' bases.  One workgroup per problem, no atomics; one host wait. */
int mlmc_density_moments_batch(int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                               const double *sigma, const double *a, const double *b, int32_t n_intervals, int32_t gauss_degree,
                               const mlmc_basis *const *test, const int32_t *K, double *out, double *mass_out,
                               double *entropy_out);
/* Seeded draws from the densities of B problems in one call (inverse-transform sampling) -- added within 8.  Problems, rule, table
 * and Q are those of mlmc_density_quantiles_batch.  Draw j (0 <= j < 2^63) of stream s (uint32) under `seed` is x_j = Q(u_j), bit
 * for bit the value of mlmc_density_quantiles_batch for the same problem, rule and p = u_j, where u_j is defined as follows.
 *   Uniform k of the stream: Philox4x32-10 (Salmon et al., SC'11; key = (low word of seed, high word of seed), key bumps
 *     0x9E3779B9 / 0xBB67AE85 per round) of the counter (i_lo, i_hi, s, 0x53414D50), i = k >> 1, gives r0 .. r3;
 *     (hi, lo) = (r0, r1) for even k, (r2, r3) for odd k; m = (hi << 20) | (lo >> 12) (52 bits); u = (2 m + 1) 2^-53.
 *     u is an odd multiple of 2^-53: 0 < u < 1 always, u is exact in fp64, and 1 - u is exact and of the same form.
 *   Without MLMC_SAMPLE_ANTITHETIC in `flags` u_j = uniform j.  With it u_j = uniform j >> 1 for even j and 1 - (uniform j >> 1)
 *     for odd j: draws 2k and 2k + 1 are an antithetic pair.
 * Problem i writes its draws first[i] .. first[i] + n[i] - 1 of stream streams[i], one problem after another in out (and their
 * u_j in u_out, which may be NULL), the layout of the points of mlmc_density_quantiles_batch.  streams [B] host uint32 (NULL:
 * stream i = i), first [B] host int64 (NULL: zeros), n [B] host int64; mem_kind applies to out and u_out.  A draw depends on
 * (seed, stream, j, flag, problem, rule) alone: not on n, on first, on the batch, on the problem's position in it or on the launch
 * geometry; first = 50, n = 100 gives elements [50, 150) of first = 0, n = 150, so a run can be continued, and split across ranks
 * by j or by stream.  Distinct streams, and distinct seeds, give independent uniforms; the draws of different problems are
 * independent unless the caller gives them one stream (then they share their u_j: comonotone draws).  Layout, conventions,
 * argument errors and no-ops as mlmc_density_quantiles_batch; in addition first[i] < 0 and first[i] + n[i] beyond int64 are errors
 * that name the problem, unknown bits in flags an error of the call.  A problem whose mass is not finite and positive gives NaN
 * for all its draws, its u_out are still the uniforms, and it is no error.  So does a problem with a NaN among its effective
 * coefficients (NaN multipliers): the clip of the exponent hides them from the mass, and this entry does not draw from what
 * is left (the one case where a draw is not the quantile entry's value).  One workgroup per (problem, share of its draws), no
 * atomics; one host wait.
 *
 * MLMC_SAMPLE_SOBOL in `flags` (this entry, mlmc_density_sample_joint_batch and mlmc_density_sample_conditional_batch; added within
 * 8) replaces the Philox uniform of (seed, stream s, index i) by coordinate d = s of point i of a scrambled Sobol' sequence:
 * randomised quasi-Monte Carlo.  Everything downstream of "the uniform" is unchanged (Q here; normcdfinv, the product, the clamp and
 * the shift in the joint entries), and without the flag every entry returns the bits it returned before the flag existed.
 *   Direction numbers: those of Joe and Kuo (2008), 52 bits, dimensions 0 .. 1023.  V[d][t] = m_{d,t+1} << (51 - t), t = 0 .. 51;
 *     dimension 0 has every m = 1; for d >= 1, with the primitive polynomial p_d of degree s (leading and trailing bits included)
 *     and the initial values m_1 .. m_s,
 *       m_k = m_{k-s} ^ (m_{k-s} << s) ^ XOR_{i=1}^{s-1} [bit (s - i) of p_d] (m_{k-i} << i).
 *     This reproduces scipy.stats.qmc.Sobol(1024, scramble=False, bits=52).
 *   Raw point: raw(d, i) = XOR { V[d][t] : bit t of i ^ (i >> 1) is set }, the Gray-code order (point 0 is 0).
 *   Scramble, always applied and keyed by `seed`: a random linear matrix scramble and a digital shift.  word52(c0, c1) is the 52-bit
 *     word (r0 << 20) | (r1 >> 12) of Philox4x32-10 (the keying by `seed` above) of the counter (c0, c1, 0, 0x534F424C).  Digit r
 *     (r = 0 .. 51) sits at bit 51 - r.  mask_r = (word52(d, r) & ~(2^(52-r) - 1) & (2^52 - 1)) | (1 << (51 - r)): random bits on
 *     the more significant digits, a one on the diagonal; bit 51 - r of S_d(raw) is the parity of mask_r & raw.  S_d is linear
 *     over GF(2), so with V'[d][t] = S_d(V[d][t]) and shift_d = word52(d, 52)
 *       m(d, i) = XOR { V'[d][t] : bit t of i ^ (i >> 1) is set } ^ shift_d,     u = (2 m + 1) 2^-53.
 *     The host scrambles the 52 direction numbers of every distinct dimension of a call once; the device only XORs.
 *   Properties.  u is an odd multiple of 2^-53: 0 < u < 1, u and 1 - u are exact and normcdfinv(u) is finite, as for the Philox
 *     uniform.  For one seed the 2^k points whose indices start at a multiple of 2^k hit every stratum [a 2^-k, (a + 1) 2^-k) of
 *     each dimension exactly once (the scramble keeps the net property).  Distinct seeds give independent randomisations: the
 *     sample standard deviation of the means of R seeds is the error estimate of randomised quasi-Monte Carlo.  The balance holds
 *     for blocks aligned to powers of two; any first and n are allowed.
 *   Here d = streams[i] (NULL: i) for problem i; in the joint and the conditional entry d = streams[k] (NULL: k) for latent normal
 *     k and z = normcdfinv(u).  Equal streams give equal coordinates (comonotone draws), as without the flag.
 *   Errors: the flag together with MLMC_SAMPLE_ANTITHETIC is an error of the call; a stream >= 1024 is an error that names the
 *     problem (here) or the latent normal; first + n > 2^52 is an error (here it names the problem).  Every other rule of the
 *     entries carries over: the draw is bit for bit mlmc_density_quantiles_batch at the returned u, first = 50, n = 100 gives
 *     elements [50, 150) of first = 0, n = 150, and no value depends on the batch, on positions, on the blocks or on the launch
 *     geometry. */
#define MLMC_SAMPLE_ANTITHETIC 1
#define MLMC_SAMPLE_SOBOL 8   /* bits 2 and 4 stay unknown */
/* The table behind MLMC_SAMPLE_SOBOL, host arithmetic only (no device, callable before mlmc_init) -- added within 8.  For the nd
 * dimensions dims[i] < 1024 (host uint32): dirs_out[i][t], t < 52, and shift_out[i].  scramble = 0: the raw Joe-Kuo V[d][t] and
 * zero shifts; scramble = 1: V'[d][t] and shift_d under `seed`, what the sampling entries upload.  nd = 0 is a no-op; nd < 0, a
 * null array, a scramble other than 0 / 1 and a dimension >= 1024 are errors. */
int mlmc_sobol_table(uint64_t seed, int32_t scramble, const uint32_t *dims, int32_t nd, uint64_t *dirs_out, uint64_t *shift_out);
int mlmc_density_sample_batch(int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                              const double *sigma, const double *a, const double *b, int32_t n_intervals, int32_t gauss_degree,
                              uint64_t seed, const uint32_t *streams, const int64_t *first, const int64_t *n, int32_t flags,
                              double *out, double *u_out, double *mass_out, int mem_kind);
/* Seeded JOINT draws of M problems through a Gaussian copula -- added within 8.  Problems, rule, table and the quantile function
 * Q_m are those of mlmc_density_quantiles_batch (lambda / sigma [M][R1max]).  With K >= 1 latent normals and a factor F [M][K] of
 * the correlation matrix of the normal scores (host, row-major; K = M and the lower Cholesky factor is the usual case, K < M a
 * low-rank factor model, K = 1 with ones gives comonotone draws), draw j (first <= j < first + n) of component m is
 *     x[m][j] = Q_m(u[m][j]),   u[m][j] = min(max(normcdf(y[m][j]), 2^-53), 1 - 2^-53),   y[m][j] = sum_k F[m][k] z[k][j].
 *   Latent normal k of draw j: u0 = uniform i of stream streams[k] (uint32 [K] host, NULL: stream k = k) under `seed`, exactly the
 *     uniform of mlmc_density_sample_batch (same Philox keying, tag word and 52-bit construction).  Without
 *     MLMC_SAMPLE_ANTITHETIC in `flags` i = j and z = normcdfinv(u0); with it i = j >> 1 and z is negated for odd j (exact: draws
 *     2k and 2k + 1 are an exact antithetic pair of normals).  u0 is an odd multiple of 2^-53, so z is always finite.
 *   The sum y runs over k ascending in the groups of four that v_mfma_f64_16x16x4_f64 consumes, from 0; padding of M, K and n to
 *     tile sizes adds exact zeros.
 *   x[m][j] is bit for bit the value of mlmc_density_quantiles_batch for problem m, the rule and p = u[m][j].
 * Every entry of F must be finite and every row must satisfy |sum_k F[m][k]^2 - 1| <= 1e-6 (otherwise the marginals would silently
 * be wrong); a violation is an error that names the row.  One n (int64 >= 0) and one first (int64 >= 0, first + n within int64) for
 * all components.  out [M][n] and u_out [M][n] (may be NULL) and z_out [K][n] (may be NULL) are host or device arrays by mem_kind,
 * column j - first of a row holds draw j; mass_out [M] (may be NULL) is host and receives the masses of the quantile entry.
 * u[m][j] depends on (seed, streams, j, flag, row m of F) alone and x[m][j] in addition on problem m and the rule: neither depends on
 * M, on the row's position, on the other rows or problems, on n, on first, on the blocks the draws are processed in or on the launch
 * geometry; first = 50, n = 100 gives columns [50, 150) of first = 0, n = 150.  With F = I the latent normals come from the same
 * uniforms as mlmc_density_sample_batch with the same seed and streams, and the joint draws equal the independent ones up to the
 * rounding of normcdf(normcdfinv(.)): a caller who wants joint and independent draws that are independent of each other gives them
 * different seeds or streams.  Argument errors and no-ops as mlmc_density_sample_batch (null arrays, M < 0, bad rule, bad mem_kind,
 * unknown flag bits; M = 0 is a no-op); K < 1, a null factor, n < 0, first < 0 and first + n beyond int64 are errors of the call;
 * n = 0 is a no-op that still returns the masses when asked.  A problem whose mass is not finite and positive, or with NaN
 * coefficients, gives a row of NaN draws, is no error, its rows of u_out / z_out are still written and the other rows are
 * unaffected.  The draws are processed in blocks of columns so that the normals and uniforms in the workspace stay within 192 MiB
 * (MLMC_JOINT_BLOCK_DRAWS in the environment, read per call, sets the block length: a test aid, no value depends on it).  No
 * atomics; one host wait. */
int mlmc_density_sample_joint_batch(int32_t M, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                                    const double *sigma, const double *a, const double *b, int32_t n_intervals, int32_t gauss_degree,
                                    int32_t K, const double *factor, uint64_t seed, const uint32_t *streams, int64_t first, int64_t n,
                                    int32_t flags, double *out, double *u_out, double *z_out, double *mass_out, int mem_kind);
/* ---- the Student-t copula (copula_t.hip) -- added within 8 -------------------------------------------------------------
 * Elementwise functions, one thread per element, unclamped; they are the definition that the sampling entry below refers to,
 * and they exist as entries so that their accuracy can be tested at chosen arguments.  dof = nu is a double in [1, 64]; what
 * depends on nu alone (the density at 0, log Gamma(nu / 2 + 1)) is made on the host once per call, in long double.
 *   mlmc_student_t_cdf: u = T_nu(y), the CDF of Student's t.  For y <= 0 it is the lower tail with RELATIVE accuracy: with t = |y|,
 *     t < min(1.2, sqrt(nu)): 1/2 - t f(0) (1 + t^2 / nu)^-(nu + 1)/2 sum_n ((nu + 1)/2)_n / (3/2)_n w^n, w = t^2 / (nu + t^2);
 *     t < sqrt(nu): the continued fraction of I_x(nu / 2, 1/2) / 2, x = nu / (nu + t^2); beyond: its positive series in x <= 1/2.
 *     For y > 0 it is 1 - T_nu(-y), one rounded subtraction, so that cdf(y) == 1 - cdf(-y) bit for bit.  0 / 1 at -inf / +inf,
 *     NaN for NaN.
 *   mlmc_chi2_mixing_scale: s = sqrt(nu / g), g the p-quantile of the chi-square law with nu degrees of freedom (Newton on the
 *     logarithm of the regularised incomplete gamma function, lower or upper by the side of p); NaN for p outside (0, 1); finite
 *     and positive for every odd multiple of 2^-53.  A standard normal times s with a uniform p is a Student-t variate.
 *   mlmc_student_t_quantile: y = T_nu^-1(p), the inverse of mlmc_student_t_cdf.  For 0 < p <= 1/2 it is -t with t >= 0 the root of
 *     T_nu(-t) = p, T_nu(-t) the lower tail above: a start value (the tail's leading term, or the Cornish-Fisher expansion about the
 *     normal quantile), then Halley steps on log T_nu(-t) - log p with both derivatives from the closed-form density, in log t
 *     from the tail start and in t otherwise, the step clamped, at most 40 steps, until a step is below 2^-30 of t (of
 *     max(t, T / density) in t, which near p = 1/2 is what one rounding of p moves the root by); a lane that does not converge
 *     returns its last iterate.  For p > 1/2 it is -quantile(1 - p), and 1 - p is exact there, so quantile(1 - p) == -quantile(p)
 *     bit for bit.  -inf at 0, +inf at 1, 0 at 1/2, NaN for NaN and for p outside [0, 1].
 * Every loop of the three has a fixed upper trip count.  n = 0 is a no-op; dof outside [1, 64] or NaN, n < 0, a null array and a bad
 * mem_kind are errors.  The arrays [n] are host or device by mem_kind. */
int mlmc_student_t_cdf(double dof, int64_t n, const double *y, double *u_out, int mem_kind);
int mlmc_student_t_quantile(double dof, int64_t n, const double *p, double *y_out, int mem_kind);
int mlmc_chi2_mixing_scale(double dof, int64_t n, const double *p, double *s_out, int mem_kind);
/* Seeded JOINT draws of M problems through a STUDENT-T copula with dof degrees of freedom -- added within 8.  Problems, rule, tables,
 * the latent normals z[k][j], the chain acc = sum_k F[m][k] z[k][j] and Q_m are those of mlmc_density_sample_joint_batch, and so is
 * every argument check, no-op, rule for degenerate problems, block rule and flag.  In addition:
 *   Mixing uniform: p0[j] = uniform i of stream mix_stream under `seed` (the Philox uniform of mlmc_density_sample_batch), or under
 *     MLMC_SAMPLE_SOBOL coordinate mix_stream (< 1024) of point j; i = j, or j >> 1 with MLMC_SAMPLE_ANTITHETIC: draws 2k and 2k + 1
 *     then share s and negate z, an exact antithetic pair in y.  mix_stream equal to one of `streams` (NULL: k) is an error.
 *   s[j] is bit for bit mlmc_chi2_mixing_scale(dof, p0[j]);  y = acc (x) s[j], ONE rounded multiplication after the chain has ended;
 *   u = min(max(T, 2^-53), 1 - 2^-53) with T bit for bit mlmc_student_t_cdf(dof, y);  x = Q_m(u), bit for bit the quantile entry.
 * s_out [n] (may be NULL) sits next to u_out and z_out (host or device by mem_kind).  u[m][j] depends on (seed, streams, mix_stream,
 * j, flags, dof, row m of F) alone: not on M, the padding of K, n, first, the blocks, the memory kind or the launch geometry;
 * first = 50, n = 100 gives columns [50, 150) of first = 0, n = 150.  dof outside [1, 64] or NaN is an error of the call.  The
 * mixing scales of a block (8 bytes per draw) live next to the normals and uniforms, beyond the 192 MiB that size the block.
 * mlmc_density_quantiles_kernel_time counts the mixing, normals, product, map and sampling kernels of a block and group as one
 * launch.  Box probabilities and event scenarios under the t copula are mlmc_copula_box_prob_t_batch / _draws_t_batch below;
 * conditional draws under a t copula are mlmc_density_sample_conditional_t_batch. */
int mlmc_density_sample_joint_t_batch(int32_t M, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                                      const double *sigma, const double *a, const double *b, int32_t n_intervals, int32_t gauss_degree,
                                      int32_t K, const double *factor, double dof, uint64_t seed, const uint32_t *streams,
                                      uint32_t mix_stream, int64_t first, int64_t n, int32_t flags, double *out, double *u_out,
                                      double *z_out, double *s_out, double *mass_out, int mem_kind);
/* Seeded CONDITIONAL joint draws under the Gaussian copula, B sets of observed values at once -- added within 8.  The M problems
 * are the UNOBSERVED components; problems, rule, table, Q_m, the latent normals z[k][j] (seed, streams, first, n, flags) and every
 * argument up to `flags` are those of mlmc_density_sample_joint_batch.  With the conditional factor F [M][K] (host, row-major; the
 * Schur-complement Cholesky block of the scores' correlation) and the conditional means shift [B][M] (host; NULL: zeros), draw j
 * of problem m in set b is
 *     x = Q_m(u),   u = min(max(normcdf(y), 2^-53), 1 - 2^-53),   y = shift[b][m] (+) acc,
 *   acc the chain of the joint entry (k ascending in the groups of four of v_mfma_f64_16x16x4_f64, from 0) and (+) ONE fp64
 *   addition rounded to nearest after the chain has ended.  x is bit for bit mlmc_density_quantiles_batch at p = u.  With a zero
 *   shift and unit rows the entry gives the bits of mlmc_density_sample_joint_batch in u, x and z (0 + (-0) = +0 does not change
 *   normcdf).
 * Every entry of F must be finite and every row must satisfy sum_k F[m][k]^2 <= 1 + 1e-6; it need not be 1 (the conditional
 * standard deviation of the score is at most 1) and a row of zeros is allowed: every draw of it is Q_m(clamp(normcdf(shift))).  A
 * violation names the row.  Every shift must be finite; a violation names set and row.  Large shifts are fine: |shift| = 40 gives
 * u = 2^-53 or 1 - 2^-53 exactly and a finite x.
 * Layout: rows [M] (host int32, strictly increasing, 0 <= rows[m] < ld_rows; NULL: the identity) and ld_rows >= M.  Draw j of
 * problem m in set b goes to out[((b * ld_rows) + rows[m]) * n + (j - first)]; u_out (may be NULL) has the same layout; rows that
 * `rows` does not name are NOT touched (the caller fills them with the observed values).  out and u_out are host or device arrays
 * by mem_kind, z_out [K][n] (may be NULL) too; mass_out [M] (may be NULL) is host.
 * u[b][m][j] depends on (seed, streams, j, flag, row m of F, shift[b][m]) alone and x in addition on problem m and the rule: neither
 * depends on B, on the position of a set, on M, on rows / ld_rows, on n, on first, on the blocks the draws are processed in or on
 * the launch geometry.  The M tables, the normals and their launch are made once per block of draws for all sets; every set forms
 * its tile of the product on the matrix cores and adds its shift.
 * The block of draws is chosen so that the normals [K][nb] and the uniforms [B * M][nb] stay within 192 MiB
 * (MLMC_JOINT_BLOCK_DRAWS as for the joint entry).  If a block of 64 draws alone exceeds that (B * M beyond about 3.9e5 rows) the
 * call is an error that says to split the sets across calls, which changes no value.
 * Argument errors, no-ops (M = 0; n = 0 still returns the masses), degenerate problems (a row of NaN draws in every set, u_out /
 * z_out still written), the one host wait and the accounting of mlmc_density_quantiles_kernel_time (one launch per block and
 * group) are those of the joint entry; B < 1, a rows array that is not strictly increasing within 0 .. ld_rows - 1, ld_rows < M
 * and B * ld_rows * n beyond int64 are errors of the call.  No atomics. */
int mlmc_density_sample_conditional_batch(int32_t M, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                                          const double *sigma, const double *a, const double *b, int32_t n_intervals,
                                          int32_t gauss_degree, int32_t K, const double *factor, uint64_t seed, const uint32_t *streams,
                                          int64_t first, int64_t n, int32_t flags, int32_t B, const double *shift, const int32_t *rows,
                                          int32_t ld_rows, double *out, double *u_out, double *z_out, double *mass_out, int mem_kind);
/* Seeded CONDITIONAL joint draws under the STUDENT-T copula, B sets of observed values at once -- added within 8.  Given the t
 * scores y_O of p observed components, the t scores of the others are multivariate t with nu + p degrees of freedom, location W y_O
 * and scale matrix g F_c F_c^T, g = (nu + d) / (nu + p), d = y_O^T C_OO^-1 y_O: an extreme observation widens the law of the
 * rest.  This entry defines the arithmetic; the caller supplies shift = W y_O, scale[b] = sqrt(g_b) and dof_mix = nu + p.
 *   Arguments, layout (rows / ld_rows), no-ops, argument errors, the rule for degenerate problems, the block rule, the workspace
 *     bound and the independence properties are those of mlmc_density_sample_conditional_batch.
 *   The mixing uniform p0[j], the rules for mix_stream (equal to one of `streams` is an error), the antithetic pairing (draws 2k and
 *     2k + 1 share s and negate z) and the handling of MLMC_SAMPLE_SOBOL are those of mlmc_density_sample_joint_t_batch.
 *   dof lies in [1, 64], dof_mix in [1, 192]; NaN is outside both: errors of the call.  dof_mix need not be dof + an integer.
 *   scale [B] (host; NULL: ones): every scale must be finite and positive; a violation names the set.
 *   s[j] is bit for bit mlmc_chi2_conditional_scale(dof_mix, p0[j]);
 *   y = shift[b][m] (+) ((acc (x) s[j]) (x) scale[b]): acc the chain of the joint entry, then THREE fp64 operations, each rounded to
 *     nearest, in this order;
 *   u = min(max(T, 2^-53), 1 - 2^-53) with T bit for bit mlmc_student_t_cdf(dof, y): the MARGINAL t CDF has dof degrees of freedom,
 *     not dof_mix;  x = Q_m(u), bit for bit mlmc_density_quantiles_batch at p = u.
 * With B = 1, NULL (or zero) shift, NULL (or unit) scale, dof_mix == dof and unit rows the entry returns the bits of
 * mlmc_density_sample_joint_t_batch in out, u_out, z_out and s_out.  s_out [n] (may be NULL; host or device by mem_kind) sits next
 * to z_out.  No value depends on B, the position of a set, M, rows / ld_rows, n, first, the block length, the memory kind or the
 * launch geometry.  The mixing scales of a block live where the joint t entry keeps them; the product and the map are kernels of
 * their own (the map runs over the rows of all sets), and mlmc_density_quantiles_kernel_time counts the kernels of a block and
 * group as one launch.  Every loop has a fixed upper trip count; no atomics; one host wait. */
int mlmc_density_sample_conditional_t_batch(int32_t M, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                                            const double *sigma, const double *a, const double *b, int32_t n_intervals,
                                            int32_t gauss_degree, int32_t K, const double *factor, double dof, double dof_mix,
                                            uint64_t seed, const uint32_t *streams, uint32_t mix_stream, int64_t first, int64_t n,
                                            int32_t flags, int32_t B, const double *shift, const double *scale, const int32_t *rows,
                                            int32_t ld_rows, double *out, double *u_out, double *z_out, double *s_out, double *mass_out,
                                            int mem_kind);
/* mlmc_chi2_mixing_scale with dof_mix in [1, 192], the range of the mixing variable of the entry above -- added within 8.  For
 * dof_mix <= 64 it gives the bits of mlmc_chi2_mixing_scale; the capped loops stay below half their caps up to 192.  It exists so
 * that the scale can be tested at chosen arguments.  Errors and no-ops are those of mlmc_chi2_mixing_scale. */
int mlmc_chi2_conditional_scale(double dof_mix, int64_t n, const double *p, double *s_out, int mem_kind);
/* Normal scores of stored samples under the densities of M problems in one call -- added within 8: the probability-integral
 * transform followed by normcdfinv, the step between the fitted marginals and a correlation of the Gaussian copula
 * (mlmc_density_sample_joint_batch).  Problems, rule, table, masses and Fhat_m are those of mlmc_density_cdf_batch (lambda / sigma
 * [M][R1max], domain [a[m], b[m]], n_intervals, gauss_degree; 0 = 64 and 21).  fine and coarse are DEVICE arrays [M][ld_in] of
 * which n columns are used, the component-major chunk layout of mlmc_accum_push; coarse may be NULL (level 0), then z_coarse and
 * u_coarse are ignored.  z_fine / z_coarse are DEVICE arrays [M][ld_out]; u_fine / u_coarse (may be NULL) have the same layout;
 * mass_out [M] host (may be NULL) receives the masses.  For component m and a value x of its row:
 *   z = u = NaN if x is NaN, if the problem's mass is not finite and positive, if one of its effective coefficients is NaN (the
 *     rule of mlmc_density_sample_batch), or if x lies outside the OPEN interval (a[m], b[m]): the end points themselves drop;
 *   otherwise u = Fhat_m(x), bit for bit the value of mlmc_density_cdf_batch for the same problem, rule and x, and
 *     z = normcdfinv(min(max(u, 2^-53), 1 - 2^-53)), the clamp of mlmc_density_sample_joint_batch (|z| <= 8.21); a u that is NaN
 *     because the density left its basis' domain inside (a, b) gives z = NaN.
 * Values outside the domain drop and are not clamped: the densities were fitted to the in-domain samples alone (the moment
 * functions mask the rest), so u is uniform on exactly those, and a NaN in any row of a column drops the sample pair in the
 * component-covariance accumulator.  The test compares the raw value with a and b; the mask of the moment functions compares the
 * transformed value with the reference domain, so at a boundary ulp the two may count a sample differently.  A value depends on
 * (problem m, rule, x) alone: not on M, on the row's position, on n, on ld_in / ld_out, on whether coarse is present or on the
 * launch geometry.  An output array may overlap neither an input array nor another output array (an error of the call, as are
 * a null array, M < 0, n < 0, ld_in < n, ld_out < n and a bad rule); errors of one problem name it as in mlmc_density_cdf_batch.
 * M = 0 is a no-op, n = 0 a no-op that still returns the masses when asked.  One thread owns the fine and the coarse value of a
 * column (without coarse: two columns), no atomics; one host wait. */
int mlmc_density_scores_batch(int32_t M, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda, const double *sigma,
                              const double *a, const double *b, int32_t n_intervals, int32_t gauss_degree, const double *fine,
                              const double *coarse, int64_t n, int64_t ld_in, double *z_fine, double *z_coarse, int64_t ld_out,
                              double *u_fine, double *u_coarse, double *mass_out);
/* HIP-event time (ms) and number of the point kernels (quantile, CDF and sampling kernels, without the table kernels and copies)
 * that mlmc_density_cdf_batch / mlmc_density_quantiles_batch / mlmc_density_tail_means_batch / mlmc_density_sample_batch /
 * mlmc_density_sample_joint_batch / mlmc_density_scores_batch have launched since the last call of this function; resets both.  A
 * tail-means call counts its quantile kernel and its tail kernel together as one launch per group; a sampling call counts its
 * sampling kernel, one launch per group; a joint sampling call counts its normals, uniforms and sampling kernels together as one
 * launch per block and group; a scores call counts its scores kernels, one launch per group. */
int mlmc_density_quantiles_kernel_time(double *ms, int64_t *launches);

/* ---- joint box probabilities under the Gaussian copula -- added within 8 ------------------------------------ */
/* P(lo < Y < hi) for Y = shift + L z, z standard normal [M], for B boxes and R seeds in one call: Genz's separation of variables
 * (Genz, J. Comput. Graph. Statist. 1, 1992) on the points of the sampling entries.  Everything is in SCORE space: the caller maps
 * limits to normal scores (mlmc_density_scores_batch) and brings the factor.
 *   L [M][M] host, row-major, lower triangular with a positive diagonal; the upper part is ignored and rows need not have unit norm
 *     (a conditional factor has not).  1 <= M <= MLMC_BOX_PROB_MAX_M.
 *   lo, hi [B][M] host, +-inf allowed; shift [B][M] host (NULL: zeros), the mean of the scores per box; seeds [R] host uint64;
 *   streams [M-1] host uint32 (NULL: i); first, n: the points first .. first + n - 1, n >= 1, first + n <= 2^52.
 *   flags: 0 or MLMC_SAMPLE_SOBOL.  With it w_i of point j under seed r is coordinate d = streams[i] of point j of the scrambled
 *     Sobol' sequence keyed by seeds[r] (above); without it the Philox uniform j of stream streams[i] under seeds[r]
 *     (mlmc_density_sample_batch).  Either is an odd multiple of 2^-53 in (0, 1).
 * The integrand of point j, box b, seed r, every operation ONE fp64 operation rounded to nearest (no FMA anywhere), f = 1 and for
 * i = 0 .. M-1:
 *     s   = shift[b][i], then for k = 0 .. i-1 ascending   s = s + (L[i][k] * y_k)      (0 without a shift)
 *     a'  = (lo[b][i] - s) / L[i][i],   b' = (hi[b][i] - s) / L[i][i]
 *     if a' > 0 (the reflected side):   d = normcdf(-b'), e = normcdf(-a'), sign = -1
 *     else:                             d = normcdf(a'),  e = normcdf(b'),  sign = +1
 *     width = e - d if lo[b][i] < hi[b][i], else 0;      f = f * width
 *     for i < M-1:   y_i = sign * normcdfinv(min(max(d + (w_i * width), 2^-1022), 1 - 2^-53))
 *   The reflection makes an upper-tail box a difference of two small numbers instead of two numbers next to 1; the clamp keeps
 *   every y finite (|y| < 37.6), so no step forms inf - inf or 0 * inf: a box with lo >= hi in some component has f = 0 exactly,
 *   an f that has become 0 stays 0 and never NaN (a box at [40, 41] gives 0), and the box (-inf, inf)^M gives exactly 1.
 * mean [R][B] host: the sum of f over the n points, divided by n.  The sum is a fixed tree: the points are taken in blocks of 64
 *   aligned to multiples of 64 of the index j; within a block, with +0 for the j outside [first, first + n), v_l += v_(l ^ 32), then
 *   ^ 16, ^ 8, ^ 4, ^ 2, ^ 1; of the blocks' sums p_0, p_1, ... thread t < 256 adds p_t, p_(t + 256), ... in ascending order from 0, and
 *   the 256 sums fold by halves (t < 128: v_t += v_(t + 128), then 64, ... 1).  The tree is fixed by (first, n) alone: mean[r][b] is
 *   bitwise repeatable, depends on (L, box b, seed r, streams, first, n, flag) alone -- not on B, on R, on the position of the box
 *   or the seed, on how the launches are split (MLMC_BOX_PROB_BLOCK_POINTS in the environment, read per call, sets the points of a
 *   launch: a test aid) -- and is the same with and without f_out.  M = 1 uses no point: mean = e - d exactly, for any n.
 * f_out [R][B][n] (may be NULL), host or device by mem_kind: the integrand, column j - first.
 * Errors: M < 1 or above the cap, B < 1, R < 1, n < 1, first < 0, first + n > 2^52, a null array, bad mem_kind, unknown bits in
 *   flags, MLMC_SAMPLE_ANTITHETIC (it does not apply), a diagonal entry that is not finite and positive or a lower entry that is
 *   not finite (names the row), a NaN limit or a shift that is not finite (names box and component), with the flag a stream
 *   >= 1024 (names the coordinate); more than 1 GiB of block sums (R * B * n / 64 doubles) or, with a host f_out, 64 points of all
 *   pairs beyond 192 MiB say to split boxes or seeds across calls, which changes no value.
 * One wave per (seed, box, block of 64 points), a lane per point, y in LDS (512 (M - 1) bytes per wave); no atomics; one host
 * wait. */
#define MLMC_BOX_PROB_MAX_M 128
int mlmc_copula_box_prob_batch(int32_t M, const double *L, int32_t B, const double *lo, const double *hi, const double *shift, int32_t R,
                               const uint64_t *seeds, const uint32_t *streams, int64_t first, int64_t n, int32_t flags, double *mean,
                               double *f_out, int mem_kind);
/* Scenarios of Y = shift + L z GIVEN lo < Y < hi, with importance weights -- added within 8: the conditioned normals y_0 .. y_{M-1}
 * of the chain above are a sequential importance sample of the truncated normal vector (the GHK sampler), every point a scenario
 * inside the box, its weight the integrand f.  M, L, B, lo, hi, shift, R, seeds, first, n, flags, mean and every argument error
 * are those of mlmc_copula_box_prob_batch; streams is [M] (NULL: i): coordinate M-1 draws the last component.  The chain is the
 * chain above operation by operation, with for EVERY i = 0 .. M-1 (i = M-1 included; the same clamp of the argument):
 *     y_i = sign * normcdfinv(min(max(d + (w_i * width), 2^-1022), 1 - 2^-53))
 *     z_i = min(max(s + (L[i][i] * y_i), lo[b][i]), hi[b][i])           (one rounded product, one rounded sum, no FMA)
 *     u_i = min(max(normcdf(z_i), 2^-53), 1 - 2^-53)                    (the clamp of mlmc_density_sample_joint_batch)
 * f_out [R][B][n] the weights, z_out and u_out (may be NULL) [R][B][M][n], column j - first; host or device arrays by mem_kind;
 * f_out and z_out must not be NULL.  mean [R][B] host.  Host outputs are staged within the 192 MiB of the entry above (the
 * weights, z and u of a launch together), split by whole blocks of 64 points.
 *   f_out and mean are bit for bit those of mlmc_copula_box_prob_batch for the same L, box, seed, first, n, flag and
 *     streams[0 .. M-2].  M = 1 draws from its one coordinate; its weight is e - d, as there.
 *   lo_i <= z_i <= hi_i for every draw of a box that is not empty, draws of weight 0 included (a width that underflowed), and every
 *     such z is finite: y is finite by the clamp and the limits only bound it.  In a component of an empty box (lo_i >= hi_i)
 *     every draw is z_i = hi_i (finite where hi_i is) and the weight is 0; the chain goes on with y_i, which stays finite.
 *   A value depends on (L, box, seed, streams, j, flag) alone: not on B, on R, on the position of the box or the seed, on first / n
 *     (first = 50, n = 100 gives the columns [50, 150) of first = 0, n = 150), on the launch split (MLMC_BOX_PROB_BLOCK_POINTS as
 *     above), on the presence of u_out or on host / device outputs.
 *   The box (-inf, inf)^M gives weights exactly 1 and z = L normcdfinv(w): plain joint draws.
 * A lane stores its z_i at consecutive j, so the stores of a wave are coalesced per component; the last y stays in a register
 * (LDS 512 (M - 1) bytes per wave and the cap as above); no atomics; one host wait. */
int mlmc_copula_box_draws_batch(int32_t M, const double *L, int32_t B, const double *lo, const double *hi, const double *shift, int32_t R,
                                const uint64_t *seeds, const uint32_t *streams, int64_t first, int64_t n, int32_t flags, double *mean,
                                double *f_out, double *z_out, double *u_out, int mem_kind);
/* ---- the two entries above under the STUDENT-T copula -- added within 8 ---------------------------------------------------
 * P(lo < Y < hi) and scenarios given lo < Y < hi for the multivariate t vector Y = s L z with dof degrees of freedom: z standard
 * normal [M], s = sqrt(nu / chi2_nu) ONE mixing scale per point (Genz and Bretz, J. Comput. Graph. Statist. 11, 2002):
 *     P(lo < Y < hi) = E_s[ P(lo / s < L z < hi / s) ],
 * one more coordinate per point for s, every limit divided by s, the rest the Gaussian chain above.  Everything is in T-SCORE space:
 * the caller maps limits to quantiles of Student's t.  M, L, B, lo, hi, R, seeds, first, n, flags, mean, f_out, z_out, u_out,
 * mem_kind, the summation tree, the staging, the split by whole blocks (MLMC_BOX_PROB_BLOCK_POINTS) and every argument error are
 * those of the Gaussian entries, with these differences:
 *   There is no shift.  dof = nu lies in [1, 64] (NaN is outside): an error of the call otherwise.
 *   streams [M-1] (draws: [M]; NULL: i) are the chain's; mix_stream is the stream of the mixing uniform, with MLMC_SAMPLE_SOBOL a
 *     dimension below 1024 that goes into the call's Sobol' table with the chain's.  mix_stream equal to a chain stream is an error
 *     that names the coordinate (so with streams = NULL it must be at least M - 1, draws: M).
 *   s_out [R][n] (may be NULL), host or device by mem_kind: the mixing scales, column j - first.  The scales of a launch (8 bytes per
 *     seed and point) are staged within the 192 MiB next to the other rows; they alone set the blocks of a launch where no
 *     other output is staged.
 * For seed r and point j, operation by operation (every one ONE fp64 operation rounded to nearest, no FMA):
 *   1. p0 = the Philox uniform j of stream mix_stream under seeds[r], or coordinate mix_stream of point j of the Sobol' sequence
 *      keyed by seeds[r];  s = chi2_mixing_scale(nu, p0), bit for bit the value of mlmc_chi2_mixing_scale.  s depends on (seed,
 *      point) alone, not on the box: it is made once per point by a kernel of its own.
 *   2. For component i:  lt = lo[b][i] / s,  ht = hi[b][i] / s  (one correctly rounded division each; an infinite limit stays
 *      infinite), then step i of the Gaussian chain exactly as it is written above with lt, ht in the place of lo[b][i], hi[b][i]
 *      and no shift (the test for an empty component is lt < ht).  f is the product of the widths.  So f[r][b][j] is bit for bit
 *      the Gaussian entry's integrand at point j for the box (lo / s_j, hi / s_j) and the same chain streams.
 *   3. Draws: the chain's normal z_i is clamped to [lt, ht] as above; the stored score is the t score
 *          y_i = min(max(z_i * s, lo[b][i]), hi[b][i])                        (one rounded product), written to z_out, and
 *          u_i = min(max(T, 2^-53), 1 - 2^-53),  T bit for bit mlmc_student_t_cdf(nu, y_i), written to u_out by a pass of its own.
 *      lo_i <= y_i <= hi_i for every draw of a box that is not empty; a component with lo_i >= hi_i gives y_i = hi_i and weight 0.
 * mean [R][B]: the tree of the Gaussian entry over f for EVERY M: under the t copula M = 1 uses its mixing point, so its mean is
 *   the tree's value and not one width.  f_out and mean of the draws entry are bit for bit those of the probability entry for the
 *   same streams[0 .. M-2] and mix_stream.  No value depends on B, R, the position of box or seed, first / n, the launch split,
 *   the presence of f_out / u_out / s_out or host / device outputs.
 * Conditional PROBABILITIES and event scenarios (a shift) under a t copula are the _tc_ entries below: their law has nu + k degrees
 * of freedom, which leaves the [1, 64] of these entries.  Conditional draws are mlmc_density_sample_conditional_t_batch, whose
 * mixing variable takes up to 192 too.  Every loop has a fixed upper trip count; no atomics; one host wait. */
int mlmc_copula_box_prob_t_batch(int32_t M, const double *L, int32_t B, const double *lo, const double *hi, double dof, int32_t R,
                                 const uint64_t *seeds, const uint32_t *streams, uint32_t mix_stream, int64_t first, int64_t n,
                                 int32_t flags, double *mean, double *f_out, double *s_out, int mem_kind);
int mlmc_copula_box_draws_t_batch(int32_t M, const double *L, int32_t B, const double *lo, const double *hi, double dof, int32_t R,
                                  const uint64_t *seeds, const uint32_t *streams, uint32_t mix_stream, int64_t first, int64_t n,
                                  int32_t flags, double *mean, double *f_out, double *z_out, double *u_out, double *s_out, int mem_kind);
/* ---- the two t entries for a CONDITIONAL law of the t copula -- added within 8 ---------------------------------------------
 * Given the t scores y_O of p components, the t scores of the others are multivariate t with nu_c = nu + p degrees of freedom,
 * location mu and scale matrix r^2 L L^T (the caller's host algebra).  With s_c = sqrt(nu_c / chi2_nu_c) ONE mixing scale per point:
 *     P(lo < Y < hi | y_O) = E_sc[ P((lo - mu) / (r s_c) < L z < (hi - mu) / (r s_c)) ],   Y = mu + r s_c L z  inside the box.
 * The arguments, the argument errors, the stream rules, the staging (192 MiB, s_out), the tree and the split are those of the
 * _t_batch entries, with these additions:
 *   dof = nu in [1, 64]: the degrees of freedom of the COPULA, with whose constants the draws' t scores are mapped to u: the
 *     marginal law of a component is t with nu, not nu_c.  dof_mix = nu_c in [1, 192]: those of the mixing variable; s is bit for
 *     bit mlmc_chi2_conditional_scale(dof_mix, p0).  NaN is outside both intervals: an error of the call.
 *   shift [B][M] (NULL: none), finite; scale [B] (NULL: ones), finite and positive: errors of the call otherwise, before any launch.
 * For box b, seed r and point j (every operation ONE fp64 operation rounded to nearest, no FMA):
 *   1. c = scale[b] * s_j, one rounded product, once per lane (scale NULL: c = s_j).
 *   2. For component i:  lt = (lo[b][i] - shift[b][i]) / c,  ht = (hi[b][i] - shift[b][i]) / c: one rounded subtraction and one
 *      IEEE division each (shift NULL: no subtraction; an infinite limit stays infinite), then step i of the Gaussian chain on
 *      (lt, ht) without a shift; the test for an empty component is lt < ht.  So f[r][b][j] is bit for bit the Gaussian entry's
 *      integrand at point j for the box (lt, ht) and the same chain streams.
 *   3. Draws: with zn the chain's normal clamped to [lt, ht],
 *          y_i = min(max(shift[b][i] + zn * c, lo[b][i]), hi[b][i])        (one rounded product, one rounded sum), to z_out, and
 *          u_i = min(max(T, 2^-53), 1 - 2^-53),  T bit for bit mlmc_student_t_cdf(dof, y_i), to u_out by the pass of the t entries.
 *      The sign of a zero score: with shift NULL no sum is taken and y_i keeps the sign of zn * c (before the clamp) as in the
 *      _t_batch entries; with a shift the sum follows IEEE (x + (-x) = +0, -0 + -0 = -0).  The clamp is fmin(fmax(y, lo), hi).
 * With shift NULL, scale NULL and dof_mix == dof every output is bit for bit that of the _t_batch entries.  mean is the tree for
 * every M (M = 1 uses its mixing point).  No value depends on B, R, the position of box or seed, first / n, the launch split, the
 * presence of f_out / u_out / s_out or host / device outputs.  Fixed trip counts; no atomics; one host wait. */
int mlmc_copula_box_prob_tc_batch(int32_t M, const double *L, int32_t B, const double *lo, const double *hi, double dof, double dof_mix,
                                  const double *shift, const double *scale, int32_t R, const uint64_t *seeds, const uint32_t *streams,
                                  uint32_t mix_stream, int64_t first, int64_t n, int32_t flags, double *mean, double *f_out,
                                  double *s_out, int mem_kind);
int mlmc_copula_box_draws_tc_batch(int32_t M, const double *L, int32_t B, const double *lo, const double *hi, double dof, double dof_mix,
                                   const double *shift, const double *scale, int32_t R, const uint64_t *seeds, const uint32_t *streams,
                                   uint32_t mix_stream, int64_t first, int64_t n, int32_t flags, double *mean, double *f_out,
                                   double *z_out, double *u_out, double *s_out, int mem_kind);
/* ---- the two t entries with a CONDITIONED LEAD component -- added within 8 ------------------------------------------------
 * The _t_batch entries sample the mixing scale s plainly: a box that only a rare s reaches is carried by a handful of points.  These
 * entries draw the lead score V = Y_0 / L_00, which is Student-t with nu degrees of freedom, INSIDE its limits by inversion, with the
 * exact weight W0 = T_nu(hi_0 / L_00) - T_nu(lo_0 / L_00).  Given V = v the mixing scale follows s^2 = (nu + v^2) / chi2_{nu+1}, and
 * given v and s the first chain normal is y_0 = v / s:
 *     P(lo < Y < hi) = E[ W0 * prod_{i >= 1} width_i ],
 * every factor O(1): the relative error does not grow with the depth of the box.  Component 0 of the CALLER'S order leads; it should
 * be the most constraining one.  The arguments, the argument errors, the staging within 192 MiB, the summation tree, the split by
 * whole blocks and the stream rules are those of the _t_batch entries, with these differences:
 *   dof = nu in [1, 64]; the mixing variable uses nu + 1 through the constants of mlmc_chi2_conditional_scale.
 *   streams [M] in BOTH entries (NULL: i): streams[0] is the lead's coordinate, streams[i], 1 <= i <= M - 2 (draws: M - 1), the
 *     chain's.  The probability entry does not read streams[M-1] unless M = 1.  mix_stream equal to a stream that is read is an error.
 *   s_out [R][B][n] (may be NULL): the scale now depends on the box.  lead_out [R][B][n] (may be NULL): the lead score v.  Both are
 *     kept per (seed, box, point) of a launch in the workspace and count towards the 192 MiB that size a launch.
 * For seed r, box b and point j (every operation ONE fp64 operation rounded to nearest, no FMA):
 *   1. p0 = the uniform of mix_stream as in the _t_batch entries; g0 = bit for bit mlmc_chi2_conditional_scale(dof + 1, p0), made
 *      once per (seed, point), not per box.
 *   2. a = lo[b][0] / L_00, bq = hi[b][0] / L_00, refl = a > 0;  d = T(refl ? -bq : a), e = T(refl ? -a : bq), T bit for bit
 *      mlmc_student_t_cdf(dof, .);  W0 = a < bq ? e - d : 0.  Once per box.
 *   3. w = the uniform of streams[0];  p = min(max(d + w * W0, 2^-1022), 1 - 2^-53);  v = bit for bit
 *      mlmc_student_t_quantile(dof, p), negated if refl;  v = min(max(v, a), bq), then min(max(v, -2^500), 2^500): v * v is finite.
 *   4. q = sqrt((dof + v * v) / (dof + 1)), a correctly rounded square root;  sc = g0 * q;  y_0 = v / sc.
 *   5. Components i = 1 .. M-1: step i of the _t_batch chain with sc in the place of s and streams[i].  g = the product of their
 *      widths, from 1 in ascending i;  f = W0 * g, ONE rounded product at the end.  So f[r][b][j] is bit for bit W0 times the
 *      Gaussian entry's integrand at point j for the factor L[1:, 1:], the box (lo[b][1:] / sc, hi[b][1:] / sc), the shift
 *      L_i0 * y_0 (one rounded product) and streams[1:].
 *   6. Draws: row 0 is min(max(v * L_00, lo[b][0]), hi[b][0]); the others as in the _t_batch entry; u_out by the same pass with dof.
 *   7. M = 1 uses no point: mean = W0 itself for every seed, f = W0.
 * An empty lead (a >= bq) gives W0 = 0, f = 0 and v = bq.  No value depends on B, R, the position of box or seed, first / n, the
 * launch split, the presence of f_out / u_out / s_out / lead_out or host / device outputs.  Fixed trip counts; no atomics; one host
 * wait.  Conditional laws (the _tc_ entries) keep plain mixing: nu + p + 1 would leave the tested range of the t functions. */
int mlmc_copula_box_prob_tl_batch(int32_t M, const double *L, int32_t B, const double *lo, const double *hi, double dof, int32_t R,
                                  const uint64_t *seeds, const uint32_t *streams, uint32_t mix_stream, int64_t first, int64_t n,
                                  int32_t flags, double *mean, double *f_out, double *s_out, double *lead_out, int mem_kind);
int mlmc_copula_box_draws_tl_batch(int32_t M, const double *L, int32_t B, const double *lo, const double *hi, double dof, int32_t R,
                                   const uint64_t *seeds, const uint32_t *streams, uint32_t mix_stream, int64_t first, int64_t n,
                                   int32_t flags, double *mean, double *f_out, double *z_out, double *u_out, double *s_out,
                                   double *lead_out, int mem_kind);
/* ---- the three probability entries with ONE FACTOR PER BOX -- added within 8 -----------------------------------------------
 * mlmc_copula_box_prob_batch, _t_batch and _tl_batch with `int64_t factor_stride` (in doubles) behind L: box b reads the factor
 * L + b * factor_stride, [M][M] row-major.  factor_stride is 0 (one factor for all boxes: the entry without _pf_, bit for bit) or
 * at least M * M; anything else is an error of the call.  The checks of the factor run on EVERY factor and name the box.  Every
 * other argument, every error, the chain, the tree, the staging and the split are those of the entry without _pf_: the three old
 * entries ARE the factor_stride = 0 case of the same host body and the same kernels.  The arithmetic of a point does not know
 * whether its factor is shared: a box with its own copy of a factor gives bit for bit what the shared call gives, and a call with B
 * different factors gives bit for bit what B calls of one box give.  A wave owns one (seed, box), so the factor stays uniform over
 * the wave.  The factors go to the device packed, so a caller's padding costs nothing there.  Under _tl_ the lead's L_00 is that of
 * the box's factor.  Made for mlmc_copula_box_order_batch (one order, so one factor, per box) and for bootstrap replicates of a
 * correlation matrix.  The draws entries and the _tc_ entries keep one shared factor. */
int mlmc_copula_box_prob_pf_batch(int32_t M, const double *L, int64_t factor_stride, int32_t B, const double *lo, const double *hi,
                                  const double *shift, int32_t R, const uint64_t *seeds, const uint32_t *streams, int64_t first, int64_t n,
                                  int32_t flags, double *mean, double *f_out, int mem_kind);
int mlmc_copula_box_prob_t_pf_batch(int32_t M, const double *L, int64_t factor_stride, int32_t B, const double *lo, const double *hi,
                                    double dof, int32_t R, const uint64_t *seeds, const uint32_t *streams, uint32_t mix_stream, int64_t first,
                                    int64_t n, int32_t flags, double *mean, double *f_out, double *s_out, int mem_kind);
int mlmc_copula_box_prob_tl_pf_batch(int32_t M, const double *L, int64_t factor_stride, int32_t B, const double *lo, const double *hi,
                                     double dof, int32_t R, const uint64_t *seeds, const uint32_t *streams, uint32_t mix_stream,
                                     int64_t first, int64_t n, int32_t flags, double *mean, double *f_out, double *s_out, double *lead_out,
                                     int mem_kind);
/* ---- Genz's variable reordering for the chain above (box_order.hip) -- added within 8 ---------------------------------------
 * For each of B boxes a greedy pivoted Cholesky factorisation of a covariance that puts the component with the smallest expected
 * conditional width first (Genz 1992; Gibson, Glasbey and Elston 1994): the chain of mlmc_copula_box_prob_pf_batch on the permuted
 * problem has the same expectation and, for heterogeneous limits under correlation, a far smaller variance.  All arrays host.
 *   C [M][M] row-major, symmetric positive definite, finite; box b reads C + b * cov_stride, cov_stride 0 (shared) or >= M * M.
 *     Column c of the symmetric matrix is read as row c.  1 <= M <= MLMC_BOX_PROB_MAX_M.
 *   lo, hi [B][M] (+-inf allowed, no NaN); shift [B][M] finite or NULL; first [B] int32 or NULL: a component forced to lead, -1: free.
 *   perm [B][M] int32: perm[b][i] = the original component at position i.  L_out [B][M][M]: the lower-triangular factor of the
 *     permuted covariance C[perm][:, perm], zeros above the diagonal.  ok [B] int32: 0 where a pivot was not positive and finite
 *     (perm is then still a permutation; L_out is not a factor).
 * With v_j = C_jj and s_j = +0 at the start, step i = 0 .. M-1, every operation ONE fp64 operation rounded to nearest (no FMA), for
 * every component j that remains:
 *     lt = lo_j - shift_j, ht = hi_j - shift_j (without a shift: the limits);  r = sqrt(v_j);  a = (lt - s_j) / r,  b = (ht - s_j) / r
 *     if a > 0:  d = normcdf(-b), e = normcdf(-a);  else  d = normcdf(a), e = normcdf(b);     w_j = e - d if lo_j < hi_j, else 0
 *   the component c with the smallest w is taken (a NaN width counts as +inf; ties go to the lowest ORIGINAL index; at step 0
 *   first[b] >= 0 wins): perm[i] = c, L_ii = r_c, a pivot v_c that is not positive and finite clears ok, and
 *     y_i = (phi(a) - phi(b)) / w,  phi(x) = exp(-0.5 * (x * x)) * 0.3989422804014327
 *   or, where w is 0 or not finite or y is NaN, the box edge nearer to 0: a if a > 0, b if b < 0, else 0.  Every other remaining j:
 *     acc = +0, then for k = 0 .. i-1 ascending  acc = acc + (L_jk * L_ck);   L_ji = (C[c][j] - acc) / L_ii
 *     v_j = v_j - (L_ji * L_ji);   s_j = s_j + (L_ji * y_i)
 * One workgroup per box, a thread per component that never moves (perm records positions; nothing is swapped), the partial rows
 * in a global workspace laid out [k][component]; bitwise repeatable; the result of a box does not depend on B, on its position or
 * on whether its covariance is shared.  Errors: M < 1 or above the cap, B < 1, a null array, a bad cov_stride, an entry of C that
 * is not finite, a NaN limit, a shift that is not finite, first outside -1 .. M-1 (each names the box).  One host wait. */
int mlmc_copula_box_order_batch(int32_t M, const double *C, int64_t cov_stride, int32_t B, const double *lo, const double *hi,
                                const double *shift, const int32_t *first, int32_t *perm, double *L_out, int32_t *ok);

/* ---- aggregates of joint scenarios (scenario.hip) -- added within 8 ----------------------------------------------------
 * Functions of the M components of one scenario, once per scenario column.  x [S][M][ld]: S >= 1 sets of M >= 1 component rows,
 * columns 0 .. n-1 are used (n >= 0, ld >= n); agg [S][Q][ld_out], ld_out >= n, columns >= n are not touched; both host or device
 * arrays by mem_kind.  Q = A + the number of bits set in extras; the rows of a set are the A linear rows, then the extra rows in
 * the order MAX, MIN, COUNT, ARGMAX, ARGMIN (the order of the bits).  Integer-valued rows are exact doubles, so every row goes
 * through mlmc_rows_weighted_sums and mlmc_percentiles_rows unchanged.
 *   linear row a (W [A][M] host, finite, A >= 0):  acc = +0.0, then for m = 0 .. M-1 ascending  acc = acc + (W[a][m] * x[m][j]):
 *     one rounded product, one rounded sum, no FMA.  Plain IEEE: a NaN draw gives NaN, 0 * inf gives NaN.  With W[a] = e_m the row
 *     equals x[m] under == (a -0.0 comes back as +0.0: +0 + (-0) = +0, the one difference in bits).
 *   MAX, ARGMAX over the components with members[m] != 0 (members [M] host uint8; NULL: all): ARGMAX is np.argmax of the member
 *     subvector mapped back to the component index -- the first NaN if there is one, else the first index attaining the maximum
 *     under > -- and MAX is x at that index, bit for bit (of -0.0 and +0.0 the first stays).  MIN, ARGMIN: the same under <.
 *   COUNT (lower, upper [M] host, either may be NULL = no limit on that side; -inf / +inf likewise): component m is inside when
 *     lower[m] < x && x < upper[m]; count[j] = the number of components with at least one finite limit that are not inside, so
 *     a NaN draw of such a component counts, and count == 0 is the box event of mlmc_copula_box_prob_batch.
 * A value depends on its own column of its own set, on W, the limits and the members alone: not on n, ld, ld_out, S, the position
 * of the set, the alignment of a row, the launch geometry or the blocks a caller walks the columns in (columns [50, 150) of a call
 * equal a call on that slice); host and device arrays give the same bits.
 * Errors: S < 1, M < 1, n < 0, A < 0, ld < n, ld_out < n, n > 2^38, null x / agg where they are not empty (W with A > 0), bad mem_kind, unknown bits in
 * extras, a weight that is not finite (names row and component), an extreme row without a member, MLMC_AGG_COUNT with lower and
 * upper both NULL, a NaN limit (names the component).  n = 0 and Q = 0 are no-ops.
 * One lane per column, the components in order with a row stride (coalesced at any alignment), up to 8 linear accumulators in
 * registers per pass over x, further linear rows in further passes; no atomics; one host wait. */
enum { MLMC_AGG_MAX = 1, MLMC_AGG_MIN = 2, MLMC_AGG_COUNT = 4, MLMC_AGG_ARGMAX = 8, MLMC_AGG_ARGMIN = 16 };
int mlmc_scenario_aggregates(const double *x, int64_t S, int32_t M, int64_t n, int64_t ld, const double *W, int32_t A,
                             const uint8_t *members, const double *lower, const double *upper, int32_t extras, double *agg,
                             int64_t ld_out, int mem_kind);
/* Weighted statistics of rows in one pass -- added within 8.  y [n_rows][ld] (columns 0 .. n-1) and the weights f [n] (NULL: every
 * weight is 1) are host or device arrays by mem_kind; c [n_rows] (NULL: zeros; finite) and the thresholds t [n_rows][P] (P >= 0, no
 * NaN) are host.  With d = y - c[r], over the columns where neither y nor f is NaN:
 *   n_used [n_rows], n_skipped [n_rows] host int64: those columns and the others;
 *   sums [n_rows][3] host: sum f, sum (f d), sum ((f d) d);
 *   tail_sums [n_rows][P][2] host: sum f 1, sum (f d) 1, the indicator y >= t for MLMC_TAIL_UPPER, y <= t for MLMC_TAIL_LOWER.
 * Give the mean of a first call as c of a second: the second moment is then a sum of terms of the size of the result.
 * Fixed order: with per = max(2048, ceil(ceil(n / 1024) / 256) * 256) columns per block, thread t < 256 of block b adds the columns
 * b per + t, + 256, ... ascending from +0; within a wave v_l += v_(l ^ 32), then ^ 16, 8, 4, 2, 1; the four waves ((w0 + w1) + w2) + w3;
 * the blocks ascending from +0.  A row's bits depend on its data, c, t and n alone: not on n_rows, its position, ld or mem_kind.
 * No floating-point atomics.  A negative or infinite weight in a used column is an error of the call, found on the device in the
 * same pass and reported after the wait.  Other errors: a negative count, ld < n, null y (unless empty) / n_used / n_skipped / sums (t and
 * tail_sums with P > 0), bad tail or mem_kind, a centre that is not finite, a NaN threshold.  n_rows = 0 and n = 0 are no-ops that
 * write zeros.  Thresholds run 8 per pass over the rows; one host wait. */
enum { MLMC_TAIL_UPPER = 0, MLMC_TAIL_LOWER = 1 };
int mlmc_rows_weighted_sums(const double *y, int64_t n_rows, int64_t n, int64_t ld, const double *f, const double *c, const double *t,
                            int32_t P, int32_t tail, int64_t *n_used, int64_t *n_skipped, double *sums, double *tail_sums,
                            int mem_kind);

/* ---- concordance counts of the components (concordance.hip) -- added within 8 -------------------------------------------
 * How often the components of a vector lie inside box events, pair by pair and all at once, for the fine and the coarse values of a
 * level: the integers from which the multilevel estimate of a joint probability P(X_a in E_a, X_b in E_b) and its variance follow
 * exactly (the level difference of an indicator product is -1, 0 or 1), e.g. the tail-dependence function of a copula.
 *   fine, coarse: DEVICE arrays [M][ld], columns 0 .. n-1 are used (the component-major chunk of mlmc_accum_push); coarse may be
 *     NULL (level 0).  0 <= M <= MLMC_CONCORDANCE_MAX_M, n >= 0, ld >= n.
 *   lower, upper [G][M] host, 1 <= G <= MLMC_CONCORDANCE_MAX_G events; -inf / +inf: no limit on that side.
 *   Component m of a value v is INSIDE event g iff lower[g][m] < v && v < upper[g][m] (the open box of
 *     mlmc_copula_box_prob_batch): NaN is never inside, a value equal to a limit is outside.
 *   A column is KEPT iff no row of fine, and of coarse when present, holds a NaN (mask_nan_samples over the [M, n, 2] chunk, the
 *     rule of the component-covariance accumulator); a dropped column contributes to nothing.
 * For a kept column, e^f_m / e^c_m the inside indicators of the fine / coarse value of component m (e^c = 0 without coarse),
 *   J^f_ab = e^f_a e^f_b, J^c_ab = e^c_a e^c_b, A^f = prod_m e^f_m, A^c = prod_m e^c_m.  The entry ADDS to caller-owned DEVICE int64
 *   counters (the caller zeroes them; a level's slice takes block after block):
 *     pair [G][3][M][M]: [g][0][a][b] += sum_j J^f, [g][1][a][b] += sum_j J^c, [g][2][a][b] += sum_j [J^f != J^c]; full symmetric
 *       matrices, the diagonal is the marginal count;
 *     all [G][3]: the same three counts for A^f, A^c;      kept [1]: the number of kept columns (may be NULL).
 *   pair or all may be NULL and is then skipped together with its work (no bit matrix, no Gram without pair).
 * kernel_ms [2] host (may be NULL): the HIP-event time in ms of the streaming kernel and of the Gram kernel of the call's first
 *   slab of columns (the columns are walked in slabs that keep the bit matrix within 256 MiB; G M n <= 2^30 is one
 *   slab); best effort, zeros when the events cannot be made.
 * Everything is integer: the counters do not depend on the launch geometry, on the slabs (MLMC_CONCORDANCE_SLAB_WORDS in the
 * environment, read per call, sets the 64-column words of a slab: a test aid), on how the caller splits the columns across calls
 * or on the order of the calls, and repeat bit for bit.  Integer atomics only (their order cannot matter).
 * Errors: M < 0, n < 0, G < 1, M or G above its cap, ld < n, null fine (unless M = 0 or n = 0), null lower / upper, pair and all
 *   both NULL, a NaN limit (names event and component).  n = 0 and M = 0 are no-ops.
 * Two kernels per slab and a one-workgroup reduction: the values are read once, a wave's ballot makes 64 columns one word
 * ([G][2][M][ceil(n / 64)] words, 1 / 64 of the input per event and side), a pair count is popcount(word_a & word_b); one host
 * wait. */
#define MLMC_CONCORDANCE_MAX_M 1024
#define MLMC_CONCORDANCE_MAX_G 16
int mlmc_concordance_counts(const double *fine, const double *coarse, int32_t M, int64_t n, int64_t ld, int32_t G, const double *lower,
                            const double *upper, int64_t *pair, int64_t *all, int64_t *kept, double *kernel_ms);

/* ---- copula log density (copula_lik.hip) -- added within 8 ---------------------------------------------------------------
 * The log density of G copula models -- Gaussian or Student-t -- at columns of uniforms, for the fine and the coarse values of a
 * level, and the sums from which the multilevel pseudo-likelihood (the mean of the log density at the samples' probability-integral
 * transforms), its variance and those of every paired difference between two models follow.
 *   A [G][M][M] host: the lower-triangular INVERSE Cholesky factor of model g's correlation matrix R_g = L L^T, A = L^-1 (what lies
 *     above the diagonal is not read);  logdet [G] host = sum_i log L_ii = log det(R_g) / 2;  dof [G] host: nu in [1, 64], or +inf for
 *     the Gaussian copula.  1 <= M <= MLMC_COPULA_LIK_MAX_M, 1 <= G <= MLMC_COPULA_LIK_MAX_G.
 *   u_fine, u_coarse [M][ld], columns 0 .. n-1 are used, HOST or DEVICE by mem_kind; u_coarse may be NULL (level 0).  n >= 0, ld >= n.
 *   A column is KEPT iff no u of it (fine, and coarse where present) is NaN, the rule of mlmc_concordance_counts.  Kept u are
 *     clamped to [2^-53, 1 - 2^-53], as in mlmc_density_scores_batch.
 * Per kept column, side and model, with v = A y (v_i = sum_{k <= i} A_ik y_k, k ascending, one rounded operation at a time) and
 * Q = sum_i v_i^2 (i ascending):
 *   Gaussian:  y = normcdfinv(u),  l = -1/2 (Q - sum_i y_i^2) - logdet, the two sums formed in the same order;
 *   t:         y bit for bit mlmc_student_t_quantile(nu, u),
 *              l = ((c - logdet) - (nu + M)/2 log1p(Q / nu)) + (nu + 1)/2 sum_i log1p(y_i^2 / nu),
 *              c = lgamma((nu + M)/2) + (M - 1) lgamma(nu / 2) - M lgamma((nu + 1)/2), on the host in long double.
 *   M = 1 (A = 1, logdet = 0) gives l = 0 for every model, and an identity A with logdet = 0 under the Gaussian model gives l = 0,
 *   both exactly.  d_g = l^f_g - l^c_g; without u_coarse l^c = 0.
 * Outputs.  kept [1] int64 host and sums [3 G + G G] host (either may be NULL): sum l^f [G], sum l^c [G], sum d [G], sum d_g d_h
 *   [G][G] over the kept columns.  Optional per-column arrays, host or device by mem_kind, rows ldo >= n apart: y_out [G][M][ldo] the
 *   scores of the fine side, ll_fine and ll_coarse [G][ldo] (ll_coarse needs u_coarse); NaN in dropped columns.
 * A value depends on its column, the model and the side alone: not on n, ld, G, the order of the models, the presence of u_coarse,
 *   mem_kind or the launch geometry.  The sums are a fixed tree set by n alone: columns 64 b .. 64 b + 63 are one block, a dropped
 *   column and a lane beyond n add +0, the block adds v += v(lane ^ 32), ^ 16, ^ 8, ^ 4, ^ 2, ^ 1; the blocks' partials are added by
 *   256 threads, thread t the partials t, t + 256, ... in ascending order from 0, and the 256 sums fold by halves (128, 64, ... 1).
 *   No floating-point atomics.  The columns go in launches of whole blocks that keep the scores within 192 MiB
 *   (MLMC_COPULA_LIK_BLOCK_POINTS in the environment, read per call, sets the columns of a launch: a test aid, no value depends
 *   on it).
 * Errors, all before anything touches the device: M or G below 1 or above its cap, a null A / logdet / dof, n < 0, ld < n, a bad
 *   mem_kind, ldo < n with an output array, ll_coarse without u_coarse, every output NULL, dof[g] neither in [1, 64] nor +inf, a
 *   logdet that is not finite, a diagonal entry of A that is not finite and positive or an entry below it that is not finite (each
 *   names the model), null u_fine with n > 0.  n = 0 sets kept and sums to 0. */
#define MLMC_COPULA_LIK_MAX_M 128
#define MLMC_COPULA_LIK_MAX_G 16
int mlmc_copula_log_density(int32_t M, int32_t G, const double *A, const double *logdet, const double *dof, const double *u_fine,
                            const double *u_coarse, int64_t n, int64_t ld, double *y_out, double *ll_fine, double *ll_coarse, int64_t ldo,
                            int64_t *kept, double *sums, int mem_kind);

/* ---- sample percentiles (Estimate.estimate_domain, mlmc/estimator.py:275-302) -------------------------- */
/* out[i] = np.percentile(x[~isnan(x)], q_percent[i]) (NumPy "linear" method), bit-identical: exact order statistics by
 * a radix select on the device + NumPy's interpolation formula.  n_valid (may be NULL) = number of non-NaN values. */
int mlmc_percentiles(const double *x, int64_t n, const double *q_percent, int32_t nq, double *out, int64_t *n_valid,
                     int mem_kind);
/* mlmc_percentiles of every row of x, in one call: row m = x[m * ld, m * ld + n), out[m * nq + i] = np.percentile of the
 * row's non-NaN values at q_percent[i], bit for bit what mlmc_percentiles gives for that row alone; n_valid [n_rows] (may be
 * NULL): each row's number of non-NaN values.  x: host or device memory (mem_kind); q_percent, out and n_valid: host.  Rows
 * up to 16384 values are sorted in LDS, longer ones go through a segmented radix select whose digits are chosen on the
 * device (global scratch at most 64 MiB, more rows are processed in groups).  The number of launches and host waits does not
 * depend on the data.  Errors: n_rows < 1, n < 1, ld < n, nq < 1, null x / q_percent / out, a percentile outside
 * [0, 100], a row without a non-NaN value (the message names the row). */
int mlmc_percentiles_rows(const double *x, int64_t n_rows, int64_t n, int64_t ld, const double *q_percent, int32_t nq,
                          double *out /* [n_rows][nq] */, int64_t *n_valid /* [n_rows], may be NULL */, int mem_kind);

/* ---- quantity expressions (mlmc/quantity/quantity.py:35-512: arithmetic, NumPy ufuncs, comparisons, select) ------
 * A lazily built Quantity tree over one storage is lowered by the host into a straight-line register program that a
 * per-sample byte-code kernel evaluates in ONE pass over the stored rows: every node of the tree is fused, nothing but
 * the result rows is written.  A register holds the fine and the coarse value of one row of one sample.
 * Comparisons follow Quantity._process_mask (:250-262): the result is one flag per sample, true only if the condition
 * holds for the fine AND the coarse value; MLMC_X_SELECT marks the flags that `Quantity.select` (:137-164) applies. */
enum {
    MLMC_X_LOAD = 0,   /* dst = stored row a                       */
    MLMC_X_CONST,      /* dst = imm                                */
    MLMC_X_STORE,      /* result row b = reg a                     */
    MLMC_X_SELECT,     /* keep the sample only if reg a != 0       */
    MLMC_X_ADD, MLMC_X_SUB, MLMC_X_MUL, MLMC_X_DIV,
    MLMC_X_MOD,        /* np.remainder (floored, sign of divisor)  */
    MLMC_X_POW, MLMC_X_MAXIMUM, MLMC_X_MINIMUM, MLMC_X_FMAX, MLMC_X_FMIN, MLMC_X_ATAN2, MLMC_X_HYPOT, MLMC_X_FMOD,
    MLMC_X_NEG, MLMC_X_ABS, MLMC_X_SQRT, MLMC_X_SQUARE, MLMC_X_RECIP, MLMC_X_EXP, MLMC_X_EXP2, MLMC_X_EXPM1,
    MLMC_X_LOG, MLMC_X_LOG2, MLMC_X_LOG10, MLMC_X_LOG1P, MLMC_X_SIN, MLMC_X_COS, MLMC_X_TAN, MLMC_X_ASIN, MLMC_X_ACOS,
    MLMC_X_ATAN, MLMC_X_SINH, MLMC_X_COSH, MLMC_X_TANH, MLMC_X_FLOOR, MLMC_X_CEIL, MLMC_X_TRUNC, MLMC_X_RINT,
    MLMC_X_SIGN, MLMC_X_CBRT,
    MLMC_X_LT, MLMC_X_LE, MLMC_X_GT, MLMC_X_GE, MLMC_X_EQ, MLMC_X_NE,   /* per-sample flag (fine AND coarse), 0.0 / 1.0 */
    MLMC_X_AND, MLMC_X_OR, MLMC_X_NOT, MLMC_X_XOR,                        /* on flags */
    MLMC_X_N_OPS
};
/* flags or-ed into `op` of an arithmetic (ADD..FMOD) or comparison instruction: the operand is `imm`, not a register */
#define MLMC_X_IMM_A 0x4000
#define MLMC_X_IMM_B 0x8000
/* chaining: the result of the latest value-producing instruction (everything but STORE / SELECT) also stays in VGPRs.
 * A_PREV / B_PREV: the operand is that result (the register index is ignored); NO_WB on a producing instruction: the
 * result is read only through such chained operands and is not written to a register (`dst` is ignored).  Optional --
 * a program without these flags computes the same rows, with every value passing through the LDS register file. */
#define MLMC_X_A_PREV 0x2000
#define MLMC_X_B_PREV 0x1000
#define MLMC_X_NO_WB 0x0800
#define MLMC_X_OP_MASK 0x07ff
typedef struct {
    uint16_t op, dst, a, b;   /* registers < n_regs; LOAD: a = input row; STORE: b = output row */
    double imm;               /* CONST value, or the immediate operand */
} mlmc_expr_instr;
#define MLMC_EXPR_MAX_REGS 16
#define MLMC_EXPR_MAX_INSTR 4096
typedef struct mlmc_expr mlmc_expr;
int mlmc_expr_create(const mlmc_expr_instr *prog, int32_t n_instr, int32_t n_regs, int32_t n_in_rows, int32_t n_out_rows,
                     mlmc_expr **out);
void mlmc_expr_destroy(mlmc_expr *e);
/* Evaluate for n samples.  rows_in: host array of n_in_rows DEVICE pointers to the first fine value of each stored
 * row; value (sample i, fine) = row[i * sample_stride], (sample i, coarse) = row[i * sample_stride + side_stride] (doubles).
 * Two layouts occur: a row uploaded on its own -- interleaved (fine, coarse) pairs [n][2], strides (2, 1), level 0 [n],
 * stride 1 -- and a row inside an uploaded storage block [n][2][M] (the layout of the reference's Memory storage and HDF5
 * `collected_values`, sample_storage.py:169-184): pointer block + m, strides (2 M, M): fine / coarse are de-interleaved on
 * the device, the host never reshuffles.
 * fine_out / coarse_out: device buffers of n_out_rows * n doubles (coarse_out ignored without has_coarse).  Without
 * MLMC_X_SELECT the result rows are [n_out_rows][n]; with it the selected samples are compacted in order and the rows
 * are [n_out_rows][*n_selected] contiguous.  n_selected (host) receives the surviving sample count; the call
 * synchronises only when the program selects. */
int mlmc_expr_eval(mlmc_expr *e, const double *const *rows_in, int32_t has_coarse, int64_t n, int64_t sample_stride,
                   int64_t side_stride, double *fine_out, double *coarse_out, int64_t *n_selected);
/* Which form evaluates this program: *state = 0 the byte-code interpreter (the program has not reached its compile threshold
 * yet), 2 its own compiled kernel (hiprtc, gfx950), -1 no compiled form (hiprtc missing, compile or load error: the
 * interpreter keeps the program), -2 compiled forms are not applicable (program too long); *compiled_launches = evaluations of
 * THIS handle that ran the compiled kernel.  Either pointer may be NULL.  (MLMC_EXPR_JIT=0 keeps the interpreter,
 * MLMC_EXPR_JIT_AFTER=k compiles at the (k+1)-th evaluation, MLMC_EXPR_JIT_VERBOSE=1 prints the hiprtc log on failure.) */
int mlmc_expr_state(mlmc_expr *e, int32_t *state, int64_t *compiled_launches);
/* HIP-event time (ms), launches and algorithmic bytes (8 B per value of every referenced stored row and every result
 * row) of the evaluation kernel since create or the previous call; same contract as mlmc_accum_kernel_time. */
int mlmc_expr_kernel_time(mlmc_expr *e, double *ms, int64_t *launches, int64_t *alg_bytes);

/* ---- bootstrap sub-sampling (Quantity.pick_samples, mlmc/quantity/quantity.py:308-325; Estimate.est_bootstrap,
 * mlmc/estimator.py:171-205) ------------------------------------------------------------------------------------
 * out[r][j] = in[r][idx_j], j < k, idx_j uniform in [0, n) with replacement (RNG.choice(chunk, size=k, axis=1)); the
 * same idx_j for every row and for fine and coarse.  idx_j comes from Philox4x32-10 keyed by `seed` with counter j, so a
 * draw is reproducible from (seed, n, k) alone; the reference's generator is an unseeded module global, parity is
 * statistical only.  All pointers are DEVICE pointers: fine / coarse [n_rows][n] (coarse may be NULL),
 * fine_out / coarse_out [n_rows][k].  Asynchronous on the library's stream. */
int mlmc_subsample_gather(const double *fine, const double *coarse, int32_t n_rows, int64_t n, int64_t k, uint64_t seed,
                          double *fine_out, double *coarse_out);

/* ---- batched, seeded bootstrap of the moment estimates (Estimate.est_bootstrap, mlmc/estimator.py:171-205) -- added within 8 ----
 * Replicate b of a chunk of n samples picks sizes[b] of them uniformly with replacement (RNG.choice(chunk, size, axis=1)): integer
 * weights w[b][0 .. n) ~ Multinomial(sizes[b], uniform), sum_i w[b][i] = sizes[b].  They are drawn exactly as a multinomial over
 * tiles of 4096 positions followed by uniform positions inside each tile, with Philox4x32-10 keyed by `seed` and a counter made of
 * (draw, replicate index, tile, stream): the weights of replicate b depend on (seed, stream, n, b, sizes[b]) only -- not on the
 * batch size or the range asked for.  `stream` tells chunks apart (mlmc_amd passes level << 20 | chunk index of the level).
 * Chunks of up to 251658240 samples, 0 <= sizes[b] <= n. */
/* The [nb][n] int32 weights of replicates b0 .. b0 + nb - 1 (sizes: host [nb]; w_out: DEVICE [nb][n]).  Synchronous. */
int mlmc_bootstrap_weights(int64_t n, int64_t b0, int64_t nb, const int64_t *sizes, uint64_t seed, uint32_t stream,
                           int32_t *w_out);
typedef struct mlmc_bootstrap mlmc_bootstrap;
/* Per-replicate level sums of the moments of a quantity with M components for B replicates and n_levels levels.  Basis: Legendre,
 * monomial or Fourier (log / safe_eval included), no transform, M * R <= 2048.  Device state: the totals [n_levels][B][2 M R]
 * doubles plus at most 64 MiB of scratch (tile counts, one weight slab, partial rows); larger B and n run in groups. */
int mlmc_bootstrap_create(const mlmc_basis *b, int32_t M, int32_t n_levels, int64_t B, mlmc_bootstrap **out);
void mlmc_bootstrap_destroy(mlmc_bootstrap *bs);
/* Zero the totals (waits for the stream). */
int mlmc_bootstrap_reset(mlmc_bootstrap *bs);
/* Add one chunk of level `level` (fine / coarse: DEVICE [M][n], coarse NULL at level 0; sizes: host [B]) with exactly the weights
 * mlmc_bootstrap_weights(n, 0, B, sizes, seed, stream) gives: per replicate b the kept count sum_i w_bi keep_i and the sums
 * sum_i w_bi d_i, sum_i w_bi d_i o d_i over the moment differences d_i (fine - coarse; level 0: fine) of all M x R rows, row
 * m * R + r.  keep_i: the sample's M fine and M coarse values all pass the basis transform (NaN / out of domain drop the whole
 * sample, as mlmc_accum_push).  Asynchronous on the library's stream; no launch depends on device results.  The buffers must
 * stay valid until mlmc_bootstrap_finalize.  Deterministic: a replicate's sums do not depend on B. */
int mlmc_bootstrap_accum(mlmc_bootstrap *bs, int32_t level, const double *fine, const double *coarse, int64_t n,
                         const int64_t *sizes, uint64_t seed, uint32_t stream);
/* Wait for the stream and write (host) n_out [B][n_levels] kept counts, s_out / sp_out [B][n_levels][M * R] sums.  The totals
 * stay (reset to start over). */
int mlmc_bootstrap_finalize(mlmc_bootstrap *bs, int64_t *n_out, double *s_out, double *sp_out);
/* With timing enabled (mlmc_init flags bit 0): HIP-event ms of the contraction launches (keep bytes, contraction, reduction) and of
 * the RNG launches (tile counts, weights), and the executed v_mfma_f64_16x16x4_f64 flops, since create or the previous call. */
int mlmc_bootstrap_kernel_time(mlmc_bootstrap *bs, double *ms_contract, double *ms_rng, int64_t *mfma_flops);
/* Per-component bootstrap -- added within 8.  A handle for M components with K moments each, component m under bases[m]: plain
 * Legendre, monomial or Fourier members of ONE family, no transform, size >= K, each with its own domain, log, x_lo / x_hi and
 * safe_eval (the rules and messages of mlmc_accum_estimate_multi; they name this entry and the component).  K in 1 .. 512,
 * M in 1 .. 65535; there is no column cap, components run in groups of at most 2048 columns.  Device state: the totals
 * [n_levels][B][M (2 K + 1)] doubles (refused above 2 GiB), the 64 MiB of scratch and at most max(8 MiB, 4096 M) keep bytes.
 * The bases must outlive the handle.  mlmc_bootstrap_accum / _reset / _destroy / _kernel_time serve the handle unchanged
 * (fine / coarse: DEVICE [M][n]; the weights are those of mlmc_bootstrap_weights); mlmc_bootstrap_finalize refuses it. */
int mlmc_bootstrap_create_multi(int32_t M, const mlmc_basis *const *bases, int32_t K, int32_t n_levels, int64_t B,
                                mlmc_bootstrap **out);
/* Wait for the stream and write (host) n_out [B][n_levels][M], s_out / sp_out [B][n_levels][M * K] (row m * K + k):
 * n = sum_i w_bi keep_im, s = sum_i w_bi keep_im d_imk, sp = sum_i w_bi keep_im d_imk^2 with d_imk = phi_k(fine_im) - phi_k(coarse_im)
 * (level 0: phi_k(fine_im)) under bases[m], and keep_im the mask mlmc_accum_push applies to a one-component chunk of row m: a
 * NaN or an out-of-domain value of component m drops the sample for component m alone.  The counts are exact.  Refuses a handle
 * of mlmc_bootstrap_create.  The totals stay (reset to start over). */
int mlmc_bootstrap_finalize_multi(mlmc_bootstrap *bs, int64_t *n_out, double *s_out, double *sp_out);
/* Component covariance of the bootstrap replicates -- added within 8.  A handle for the M components of a vector quantity
 * (M in 1 .. 1024, no basis): per replicate b and level l, with the weights w_b of mlmc_bootstrap_weights, a shift a [M] and
 * f~ = f - a, c~ = c - a (both rounded to fp64),
 *     n = sum_i w_bi keep_i,   s1[m] = sum_i w_bi keep_i (f~_im - c~_im),   s2[i][j] = sum_i w_bi keep_i (f~_i f~_j - c~_i c~_j)
 * (level 0 / coarse NULL: f~_im and f~_i f~_j), keep_i = 0 when any of the sample's M fine or M coarse values is NaN: the rule of
 * mlmc_xcov_create, the sample is dropped from the whole matrix and contributes exact zeros.  No sums of squares: the replicates
 * are the error estimate.  Device state: the totals [n_levels][B][1 + M + M (M + 1) / 2] doubles (refused above 2 GiB) and the
 * 64 MiB of scratch; the columns run in groups of at most 2048.  mlmc_bootstrap_accum / _reset / _destroy / _kernel_time serve
 * the handle unchanged (fine / coarse: DEVICE [M][n]); mlmc_bootstrap_finalize and mlmc_bootstrap_finalize_multi refuse it.
 * Deterministic: runs are bit-identical and a replicate's sums do not depend on B. */
int mlmc_bootstrap_create_xcov(int32_t M, int32_t n_levels, int64_t B, mlmc_bootstrap **out);
/* The shift a (host, M finite doubles; NULL: zeros) of a handle of mlmc_bootstrap_create_xcov.  It takes effect at the next
 * mlmc_bootstrap_reset; an error while chunks have been accumulated since the last reset (the rule of mlmc_xcov_set_shift). */
int mlmc_bootstrap_set_shift(mlmc_bootstrap *bs, const double *shift_host);
/* Wait for the stream and write (host) n_out [B][n_levels], s1_out [B][n_levels][M], s2_out [B][n_levels][M * M] (row i * M + j,
 * bitwise symmetric: one computed value goes to (i, j) and (j, i)).  The counts are exact.  Refuses the handles of
 * mlmc_bootstrap_create and mlmc_bootstrap_create_multi.  The totals stay (reset to start over). */
int mlmc_bootstrap_finalize_xcov(mlmc_bootstrap *bs, int64_t *n_out, double *s1_out, double *s2_out);

/* ---- synthetic samples in HBM (mlmc/sim/synth_simulation.py:37-46,75-131; seeding mlmc/sampling_pool.py:75-84; sample
 * ids mlmc/sampler.py:120) -------------------------------------------------------------------------------------------
 * Samples first_sample .. first_sample + n - 1 of level `level_id` exactly as Sampler + SynthSimulation (distr =
 * scipy.stats.norm(loc, scale), result_format of synth_simulation.py:136-145: 24 stored rows) produce them: md5 of the sample id
 * -> MT19937 -> two legacy Box-Muller normals -> x + h sqrt(1e-4 + |x|).  rows (host array): the stored rows wanted
 * (0..23 = [quantity][time][location][component]); out (host array of DEVICE pointers): one buffer per row in the
 * storage layout -- interleaved (fine, coarse) pairs [n][2] when coarse_step != 0, else fine only [n] (level 0).
 * Asynchronous on the library's stream. */
int mlmc_synth_generate(int32_t level_id, int64_t first_sample, int64_t n, double fine_step, double coarse_step,
                        double loc, double scale, int32_t n_rows, const int32_t *rows, double *const *out);
/* seeds_host[i] = SamplingPool.compute_seed("L{level:02d}_S{first + i:07d}") (first uint32 of the md5 digest); synchronous */
int mlmc_synth_seeds(int32_t level_id, int64_t first_sample, int64_t n, uint32_t *seeds_host);

#ifdef __cplusplus
}
#endif
#endif /* MLMC_HIP_H */
