// mlmc_copula_log_density (include/mlmc_hip.h): the log density of Gaussian and Student-t copulas at columns of uniforms, for G
// models at once, fine against coarse, with the sums of a multilevel pseudo-likelihood (gfx950).
//
//   k_lik_normal_scores : Y = normcdfinv(clamp(U)), NaN for NaN, one thread per element: the scores of a Gaussian model.  The t
//                 scores of a model with finite nu are k_tcop_scores (copula_t.hip).  Both are passes of their own ahead of the
//                 chain: the series loops and constants of the quantiles stay out of the loop over i.
//   k_lik_chain : one workgroup of ONE wave owns 64 consecutive columns of one model (grid: blocks x models); a lane owns one
//                 column and runs, for the fine and then the coarse side, the triangular product v = A y of the header row by row:
//                 the lane's y_0 .. y_{M-2} live in LDS as y[k][lane] (dynamic, 512 (M - 1) bytes per workgroup; the cap M = 128
//                 takes 65024 bytes), the last y stays in a register; a lane reads back only what it wrote itself, so the chain
//                 needs no barrier.  The rows of A and the model's constants are uniform over the wave: scalar loads.  Q = sum v_i^2
//                 and sum y_i^2 (Gaussian) or sum log1p(y_i^2 / nu) (t) are formed in the same order, one rounded operation at a
//                 time.  A column with a NaN score on either side is dropped: NaN in both of its log densities (and, when the
//                 caller asked for the scores, in its fine scores).
//   k_lik_gram  : one wave per 64 columns: d_g = l^f_g - l^c_g of every model in LDS as d[g][lane], then the wave's butterfly over
//                 its columns for each statistic: sum l^f_g, sum l^c_g, sum d_g, sum d_g d_h (h <= g, stored to both places) and the
//                 number of kept columns (a sum of ones: exact); lane 0 stores the block's partials.
//   k_lik_sum   : one workgroup per statistic sums the partials of the call's blocks in a fixed tree.
// The tree: dropped columns and lanes beyond n add +0; the wave adds v += v(lane ^ 32), ^ 16, ^ 8, ^ 4, ^ 2, ^ 1; thread t of
// k_lik_sum adds the partials t, t + 256, ... in ascending order from 0 and the 256 sums fold by halves (128, 64, ... 1).  It is
// fixed by n alone.  Launches are split by whole blocks, so no value depends on the split.  No floating-point atomics.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "copula.hpp"

namespace mlmc {

constexpr int LIK_LANES = 64;                          // columns of a block = lanes of its wave
constexpr int LIK_THREADS = 256;                       // k_lik_normal_scores, k_lik_sum
constexpr int LIK_CONST = 4;                           // per model: nu (+inf: Gaussian), c_g, logdet, (nu + M) / 2
constexpr size_t LIK_WS_BYTES = (size_t)192 << 20;     // the staged uniforms, the scores and the log densities of a launch
constexpr size_t LIK_PARTIAL_BYTES = (size_t)1 << 30;  // the partials of a call

__global__ __launch_bounds__(LIK_THREADS) void k_lik_normal_scores(int64_t ncols, const double *__restrict__ U, int64_t ldu,
                                                                   double *__restrict__ Y, int64_t ldy) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncols) return;
    const double u = U[(int64_t)blockIdx.y * ldu + c];
    Y[(int64_t)blockIdx.y * ldy + c] = u != u ? u : normcdfinv(fmin(fmax(u, 0x1p-53), 1.0 - 0x1p-53));
}

// Called, not inlined (box_prob.hip): inlined into the loop over i its constants would stay in registers across the dot products.
__device__ __attribute__((noinline)) double lik_log1p(double x) { return log1p(x); }

// grid (blocks of the launch, models).  Y [G][S][M][ldy] (S = 2 with a coarse side), LL [G][S][ldy]; columns c < ncols are used.
template <bool COARSE>
__global__ __launch_bounds__(LIK_LANES) void k_lik_chain(int M, const double *__restrict__ A, const double *__restrict__ cst,
                                                         double *__restrict__ Y, int64_t ldy, int64_t ncols, double *__restrict__ LL,
                                                         int mark_scores) {
    extern __shared__ double ys[];                     // y[k][lane]
    constexpr int S = COARSE ? 2 : 1;
    const int lane = threadIdx.x, g = blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * LIK_LANES + lane;
    const bool active = c < ncols;
    const double *Ag = A + (int64_t)g * M * M;
    const double nu = cst[g * LIK_CONST], cg = cst[g * LIK_CONST + 1], logdet = cst[g * LIK_CONST + 2], half_nm = cst[g * LIK_CONST + 3];
    const bool gauss = nu == __builtin_inf();
    double ll[S];
    bool bad = false;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const double *Ys = Y + ((int64_t)(g * S + s) * M) * ldy + c;
        double Q = 0.0, P = 0.0;
        for (int i = 0; i < M; ++i) {
            const double *Ai = Ag + (int64_t)i * M;
            const double y = active ? Ys[(int64_t)i * ldy] : 0.0;
            bad = bad || y != y;
            double v = 0.0;
            for (int k = 0; k < i; ++k) v = __dadd_rn(v, __dmul_rn(Ai[k], ys[k * LIK_LANES + lane]));
            v = __dadd_rn(v, __dmul_rn(Ai[i], y));
            Q = __dadd_rn(Q, __dmul_rn(v, v));
            const double y2 = __dmul_rn(y, y);
            P = __dadd_rn(P, gauss ? y2 : lik_log1p(y2 / nu));
            if (i < M - 1) ys[i * LIK_LANES + lane] = y;
        }
        if (gauss)
            ll[s] = __dadd_rn(__dmul_rn(-0.5, __dadd_rn(Q, -P)), -logdet);
        else
            ll[s] = __dadd_rn(__dadd_rn(__dadd_rn(cg, -logdet), -__dmul_rn(half_nm, lik_log1p(Q / nu))), __dmul_rn(0.5 * (nu + 1.0), P));
    }
    if (!active) return;
    const double nan = __builtin_nan("");
#pragma unroll
    for (int s = 0; s < S; ++s) LL[(int64_t)(g * S + s) * ldy + c] = bad ? nan : ll[s];
    if (bad && mark_scores) {
        double *Yf = Y + ((int64_t)(g * S) * M) * ldy + c;
        for (int i = 0; i < M; ++i) Yf[(int64_t)i * ldy] = nan;
    }
}

__device__ __forceinline__ double lik_wave_sum(double v) {
#pragma unroll
    for (int o = LIK_LANES / 2; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// grid (blocks of the launch).  partials [3 G + G G + 1][call_blocks]: sum l^f [G], sum l^c [G], sum d [G], sum d_g d_h [G][G], kept
template <bool COARSE>
__global__ __launch_bounds__(LIK_LANES) void k_lik_gram(int G, const double *__restrict__ LL, int64_t ldy, int64_t ncols, int64_t blk0,
                                                        int64_t call_blocks, double *__restrict__ partials) {
    __shared__ double d[MLMC_COPULA_LIK_MAX_G][LIK_LANES];
    constexpr int S = COARSE ? 2 : 1;
    const int lane = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x * LIK_LANES + lane, blk = blk0 + blockIdx.x;
    // a dropped column has NaN in every log density
    const bool keep = c < ncols && LL[c] == LL[c];
    for (int g = 0; g < G; ++g) {
        const double lf = keep ? LL[(int64_t)(g * S) * ldy + c] : 0.0;
        const double lc = COARSE && keep ? LL[(int64_t)(g * S + 1) * ldy + c] : 0.0;
        const double dg = keep ? lf - lc : 0.0;
        d[g][lane] = dg;
        const double sf = lik_wave_sum(lf), sc = lik_wave_sum(lc), sd = lik_wave_sum(dg);
        if (lane == 0) {
            partials[(int64_t)g * call_blocks + blk] = sf;
            partials[(int64_t)(G + g) * call_blocks + blk] = sc;
            partials[(int64_t)(2 * G + g) * call_blocks + blk] = sd;
        }
    }
    // a lane reads back only what it wrote itself: no barrier
    for (int g = 0; g < G; ++g)
        for (int h = 0; h <= g; ++h) {
            const double v = lik_wave_sum(d[g][lane] * d[h][lane]);
            if (lane == 0) {
                partials[(int64_t)(3 * G + g * G + h) * call_blocks + blk] = v;
                partials[(int64_t)(3 * G + h * G + g) * call_blocks + blk] = v;
            }
        }
    const double k = lik_wave_sum(keep ? 1.0 : 0.0);
    if (lane == 0) partials[(int64_t)(3 * G + G * G) * call_blocks + blk] = k;
}

__global__ __launch_bounds__(LIK_THREADS) void k_lik_sum(const double *__restrict__ partials, int64_t call_blocks, double *__restrict__ out) {
    __shared__ double sh[LIK_THREADS];
    const int t = threadIdx.x;
    const double *p = partials + (int64_t)blockIdx.x * call_blocks;
    double acc = 0.0;
    for (int64_t k = t; k < call_blocks; k += LIK_THREADS) acc += p[k];
    sh[t] = acc;
    __syncthreads();
    for (int s = LIK_THREADS / 2; s; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    if (t == 0) out[blockIdx.x] = sh[0];
}

}  // namespace mlmc

using namespace mlmc;

extern "C" {

int mlmc_copula_log_density(int32_t M, int32_t G, const double *A, const double *logdet, const double *dof, const double *u_fine,
                            const double *u_coarse, int64_t n, int64_t ld, double *y_out, double *ll_fine, double *ll_coarse, int64_t ldo,
                            int64_t *kept, double *sums, int mem_kind) {
    MLMC_API_GUARD;
    const std::string e("mlmc_copula_log_density");
    if (!rt().ready) return fail("mlmc_init has not been called (no HIP device bound)");
    if (M < 1) return fail(e + ": M < 1");
    if (M > MLMC_COPULA_LIK_MAX_M) return fail(e + ": M = " + std::to_string(M) + " is above the cap " + std::to_string(MLMC_COPULA_LIK_MAX_M));
    if (G < 1) return fail(e + ": G < 1");
    if (G > MLMC_COPULA_LIK_MAX_G) return fail(e + ": G = " + std::to_string(G) + " is above the cap " + std::to_string(MLMC_COPULA_LIK_MAX_G));
    if (!A || !logdet || !dof) return fail(e + ": null model argument (A, logdet, dof)");
    if (n < 0) return fail(e + ": n < 0");
    if (ld < n) return fail(e + ": row stride ld = " + std::to_string(ld) + " is below n = " + std::to_string(n));
    if (mem_kind != MLMC_HOST && mem_kind != MLMC_DEVICE) return fail(e + ": bad mem_kind");
    const bool outs = y_out || ll_fine || ll_coarse;
    if (outs && ldo < n) return fail(e + ": output stride ldo = " + std::to_string(ldo) + " is below n = " + std::to_string(n));
    if (ll_coarse && !u_coarse) return fail(e + ": ll_coarse without u_coarse");
    if (!outs && !kept && !sums) return fail(e + ": every output is null");
    for (int g = 0; g < G; ++g) {
        if (!(dof[g] == INFINITY || (dof[g] >= 1.0 && dof[g] <= (double)TCOP_MAX_DOF)))
            return fail(e + ": model " + std::to_string(g) + ": dof must lie in [1, " + std::to_string(TCOP_MAX_DOF) + "] or be +inf");
        if (!std::isfinite(logdet[g])) return fail(e + ": model " + std::to_string(g) + ": logdet is not finite");
        const double *Ag = A + (size_t)g * M * M;
        for (int i = 0; i < M; ++i) {
            const double dg = Ag[(size_t)i * M + i];
            if (!std::isfinite(dg) || !(dg > 0.0))
                return fail(e + ": model " + std::to_string(g) + ", factor row " + std::to_string(i) +
                            ": the diagonal entry must be finite and positive");
            for (int k = 0; k < i; ++k)
                if (!std::isfinite(Ag[(size_t)i * M + k]))
                    return fail(e + ": model " + std::to_string(g) + ", factor row " + std::to_string(i) + ": entry " + std::to_string(k) +
                                " is not finite");
        }
    }
    const int n_stats = 3 * G + G * G + 1;
    if (n == 0) {
        if (kept) *kept = 0;
        if (sums) std::fill(sums, sums + (n_stats - 1), 0.0);
        return 0;
    }
    if (!u_fine) return fail(e + ": null u_fine");

    const int S = u_coarse ? 2 : 1;
    const int64_t call_blocks = (n + LIK_LANES - 1) / LIK_LANES;
    if ((double)n_stats * (double)call_blocks * sizeof(double) > (double)LIK_PARTIAL_BYTES)
        return fail(e + ": the partial sums of n / 64 blocks exceed 1 GiB: split the columns across calls");
    // blocks of a launch: what keeps the staged uniforms (host u), the scores and the log densities within LIK_WS_BYTES
    // (MLMC_COPULA_LIK_BLOCK_POINTS in the environment, read per call, sets the columns of a launch, rounded up to whole blocks: a
    // test aid, no value depends on it)
    const bool host = mem_kind == MLMC_HOST;
    const size_t rows_block = (host ? (size_t)S * M : 0) + (size_t)G * S * M + (size_t)G * S;
    int64_t lb = std::min<int64_t>(call_blocks, (int64_t)(LIK_WS_BYTES / (sizeof(double) * LIK_LANES * rows_block)));
    if (const char *env = std::getenv("MLMC_COPULA_LIK_BLOCK_POINTS")) {
        const long long v = std::atoll(env);
        if (v > 0) lb = std::min<int64_t>(lb, (v + LIK_LANES - 1) / LIK_LANES);
    }
    const int64_t W = lb * LIK_LANES;

    // what goes up: A | the constants of the models
    const size_t nA = (size_t)G * M * M;
    std::vector<double> packed(nA + (size_t)G * LIK_CONST);
    std::memcpy(packed.data(), A, sizeof(double) * nA);
    for (int g = 0; g < G; ++g) {
        double *c = packed.data() + nA + (size_t)g * LIK_CONST;
        const long double nu = dof[g];
        // c_g = lgamma((nu + M) / 2) + (M - 1) lgamma(nu / 2) - M lgamma((nu + 1) / 2) in long double; exactly 0 for M = 1
        long double cg = 0.0L;
        if (dof[g] != INFINITY && M > 1)
            cg = std::lgamma(0.5L * (nu + M)) + (long double)(M - 1) * std::lgamma(0.5L * nu) - (long double)M * std::lgamma(0.5L * (nu + 1.0L));
        c[0] = dof[g], c[1] = (double)cg, c[2] = logdet[g], c[3] = dof[g] == INFINITY ? 0.0 : 0.5 * (dof[g] + (double)M);
    }
    const size_t b_in = mm_align(sizeof(double) * packed.size()), b_part = mm_align(sizeof(double) * (size_t)n_stats * (size_t)call_blocks);
    const size_t b_sum = mm_align(sizeof(double) * (size_t)n_stats), b_u = host ? mm_align(sizeof(double) * (size_t)S * M * (size_t)W) : 0;
    const size_t b_y = mm_align(sizeof(double) * (size_t)G * S * M * (size_t)W), b_ll = mm_align(sizeof(double) * (size_t)G * S * (size_t)W);
    static MultiWorkspace ws;
    if (ws.reserve(b_in + b_part + b_sum + b_u + b_y + b_ll)) return 1;
    double *d_in = (double *)ws.dev, *d_part = (double *)(ws.dev + b_in), *d_sum = (double *)(ws.dev + b_in + b_part);
    double *d_u = (double *)(ws.dev + b_in + b_part + b_sum), *d_y = (double *)(ws.dev + b_in + b_part + b_sum + b_u);
    double *d_ll = (double *)(ws.dev + b_in + b_part + b_sum + b_u + b_y);
    hipStream_t st = rt().stream;
    MLMC_HIP_CHECK(hipMemcpyAsync(d_in, packed.data(), sizeof(double) * packed.size(), hipMemcpyHostToDevice, st));
    const double *d_A = d_in, *d_cst = d_in + nA;
    std::vector<TCopConst> tconst((size_t)G);
    for (int g = 0; g < G; ++g)
        if (dof[g] != INFINITY) tconst[g] = tcop_constants(dof[g]);

    const hipMemcpyKind down = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const size_t lds = sizeof(double) * LIK_LANES * (size_t)(M - 1);
    for (int64_t k0 = 0; k0 < call_blocks; k0 += lb) {
        const int64_t kb = std::min(lb, call_blocks - k0), c0 = k0 * LIK_LANES, nc = std::min<int64_t>(n - c0, kb * LIK_LANES);
        const double *us[2] = {u_fine + c0, u_coarse ? u_coarse + c0 : nullptr};
        int64_t ldu = ld;
        if (host) {
            for (int s = 0; s < S; ++s) {
                MLMC_HIP_CHECK(hipMemcpy2DAsync(d_u + (size_t)s * M * W, sizeof(double) * (size_t)W, us[s], sizeof(double) * (size_t)ld,
                                                sizeof(double) * (size_t)nc, (size_t)M, hipMemcpyHostToDevice, st));
                us[s] = d_u + (size_t)s * M * W;
            }
            ldu = W;
        }
        const dim3 sgrid((unsigned)((nc + LIK_THREADS - 1) / LIK_THREADS), (unsigned)M);
        for (int g = 0; g < G; ++g)
            for (int s = 0; s < S; ++s) {
                double *y = d_y + ((size_t)(g * S + s) * M) * W;
                if (dof[g] == INFINITY)
                    hipLaunchKernelGGL(k_lik_normal_scores, sgrid, dim3(LIK_THREADS), 0, st, nc, us[s], ldu, y, W);
                else
                    cop_launch_t_scores(st, tconst[g], (int)M, nc, us[s], ldu, y, W);
            }
        const dim3 cgrid((unsigned)kb, (unsigned)G);
        if (u_coarse) {
            hipLaunchKernelGGL(k_lik_chain<true>, cgrid, dim3(LIK_LANES), lds, st, (int)M, d_A, d_cst, d_y, W, nc, d_ll, (int)(y_out != nullptr));
            hipLaunchKernelGGL(k_lik_gram<true>, dim3((unsigned)kb), dim3(LIK_LANES), 0, st, (int)G, (const double *)d_ll, W, nc, k0, call_blocks,
                               d_part);
        } else {
            hipLaunchKernelGGL(k_lik_chain<false>, cgrid, dim3(LIK_LANES), lds, st, (int)M, d_A, d_cst, d_y, W, nc, d_ll, (int)(y_out != nullptr));
            hipLaunchKernelGGL(k_lik_gram<false>, dim3((unsigned)kb), dim3(LIK_LANES), 0, st, (int)G, (const double *)d_ll, W, nc, k0, call_blocks,
                               d_part);
        }
        MLMC_HIP_CHECK(hipGetLastError());
        if (y_out)
            for (int g = 0; g < G; ++g)
                MLMC_HIP_CHECK(hipMemcpy2DAsync(y_out + (size_t)g * M * ldo + c0, sizeof(double) * (size_t)ldo, d_y + ((size_t)g * S * M) * W,
                                                sizeof(double) * (size_t)W, sizeof(double) * (size_t)nc, (size_t)M, down, st));
        if (ll_fine)
            MLMC_HIP_CHECK(hipMemcpy2DAsync(ll_fine + c0, sizeof(double) * (size_t)ldo, d_ll, sizeof(double) * (size_t)S * W,
                                            sizeof(double) * (size_t)nc, (size_t)G, down, st));
        if (ll_coarse)
            MLMC_HIP_CHECK(hipMemcpy2DAsync(ll_coarse + c0, sizeof(double) * (size_t)ldo, d_ll + W, sizeof(double) * (size_t)S * W,
                                            sizeof(double) * (size_t)nc, (size_t)G, down, st));
    }
    std::vector<double> out((size_t)n_stats);
    if (kept || sums) {
        hipLaunchKernelGGL(k_lik_sum, dim3((unsigned)n_stats), dim3(LIK_THREADS), 0, st, (const double *)d_part, call_blocks, d_sum);
        MLMC_HIP_CHECK(hipGetLastError());
        MLMC_HIP_CHECK(hipMemcpyAsync(out.data(), d_sum, sizeof(double) * (size_t)n_stats, hipMemcpyDeviceToHost, st));
    }
    MLMC_HIP_CHECK(wait_stream(st));
    if (sums) std::memcpy(sums, out.data(), sizeof(double) * (size_t)(n_stats - 1));
    if (kept) *kept = (int64_t)out[(size_t)n_stats - 1];
    return 0;
}

}  // extern "C"
