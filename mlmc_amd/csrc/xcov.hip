// Multilevel covariance between the components of a vector quantity on the fp64 matrix cores (v_mfma_f64_16x16x4_f64), gfx950.
//
// Estimator (mlmc_hip.h, mlmc_xcov_create): a quantity of M scalar components, a shift a in R^M (the same for every level and
// for fine and coarse), per kept sample k of level l
//     Y_k = (f_k - a)(f_k - a)^T - (c_k - a)(c_k - a)^T          (level 0 / no coarse values: Y_k = (f_k - a)(f_k - a)^T)
// and the level sums s_l = sum_k Y_k, sp_l = sum_k Y_k o Y_k (both M x M, symmetric).  A sample is dropped from the whole
// matrix if any of its M fine or M coarse values is NaN (quantity_estimate.py:6-14, mask_nan_samples over [M, n, 2]).
//
// With d = f~ - c~ and s = f~ + c~ (f~ = f - a, c~ = c - a) -- the identities of the moment covariance (cov.hip):
//     sum Y     = 1/2 (D^T S + S^T D)
//     sum Y o Y = 1/4 (G1 + G1^T + 2 G2),   G1 = (D o D)^T (S o S),   G2 = (D o S)^T (D o S)
// Level 0: sum Y = F~^T F~, sum Y o Y = (F~ o F~)^T (F~ o F~).  The operands are the stored component values: chunks are read
// in place ([M][n], component-major, the layout mlmc_accum_push takes), the shift is subtracted and the mask applied in
// registers on the way into LDS; nothing but the partial Gram blocks is written to HBM.
//
// Tiling: the M x M output is cut into NT x NT blocks, NT = 16 T (T = 1 for M <= 16, 2 for M <= 32, else 4; ragged M is padded
// with zeros in registers).  Only the NB (NB + 1) / 2 upper blocks (bi <= bj) are computed: the two mixed products of the mean
// (D_I^T S_J + S_I^T D_J) and of G1 (DD_I^T SS_J + SS_I^T DD_J) go into ONE accumulator each, so an upper block of the
// symmetric results needs no lower block; G2 and level 0 are symmetric Grams.  MFMAs per tile and 4 samples: 5 (pair level,
// with variances), 2 (pair level, mean only; level 0 with variances), 1 (level 0, mean only).
// One launch per chunk covers every block: grid (sample slice, block pair); a 256-thread workgroup walks batches of 128 / T
// samples of its slice, four waves each own a tile row (T = 4) or a k-slice of one tile row (T < 4).  Per workgroup the
// partial Gram block goes to a scratch row; one fixed-order reduction per chunk folds the rows into the level totals and writes
// the upper entry and its mirror with the same value, so s and sp are bitwise symmetric.
// Scratch bound: the number of sample slices is chosen so that the partial rows of a launch never exceed XCOV_SCRATCH_BYTES
// (64 MiB; M = 1024 with variances: 136 block pairs x 3 Grams x 64 x 64 doubles = 13.4 MB per slice -> 4 slices, 544
// workgroups).  With M > one block (NB > 1) a pre-pass writes one keep byte per sample (k_xcov_mask); with one block the
// workgroup sees every component and decides in LDS.
// Determinism: fixed grid for a given (M, n), fixed-order reductions, no floating-point atomics; counts are integer sums.
#include <cmath>
#include <string>

#include "device_basis.hpp"

namespace mlmc {

typedef double v4f64 __attribute__((ext_vector_type(4)));

constexpr size_t XCOV_SCRATCH_BYTES = (size_t)64 << 20;

__host__ __device__ constexpr int xcov_T(int M) { return M <= 16 ? 1 : (M <= 32 ? 2 : 4); }
__host__ __device__ constexpr int xcov_ng(bool pair, bool var) { return var ? (pair ? 3 : 2) : 1; }

// block pair p (0 .. NB (NB + 1) / 2 - 1, row-major over the upper triangle) -> (bi, bj), bi <= bj
__device__ __forceinline__ void xcov_block(int p, int NB, int &bi, int &bj) {
    bi = 0;
    while (p >= NB - bi) {
        p -= NB - bi;
        ++bi;
    }
    bj = bi + p;
}

// keep byte per sample: no NaN among the M fine and (pair levels) M coarse values
__global__ __launch_bounds__(256) void k_xcov_mask(const double *__restrict__ fine, const double *__restrict__ coarse, int64_t n,
                                                   int M, uint8_t *__restrict__ mask) {
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
        bool keep = true;
#pragma unroll 8
        for (int m = 0; m < M; ++m) {
            const double v = fine[(int64_t)m * n + idx];
            keep = keep && !(v != v);
        }
        if (coarse) {
#pragma unroll 8
            for (int m = 0; m < M; ++m) {
                const double v = coarse[(int64_t)m * n + idx];
                keep = keep && !(v != v);
            }
        }
        mask[idx] = keep ? 1 : 0;
    }
}

// grid (slices, block pairs), 256 threads.  partials: row ((pair * slices + slice) * NSL + kslice) of NG x NT x NT doubles.
// pcounts (block pair 0 only): [slice][kept, removed].
template <int T, bool PAIR, bool VAR>
__global__ __launch_bounds__(256, 2) void k_xcov_accum(const double *__restrict__ fine, const double *__restrict__ coarse,
                                                       const uint8_t *__restrict__ mask, const double *__restrict__ shift,
                                                       int64_t n, int M, int NB, double *__restrict__ partials,
                                                       int64_t *__restrict__ pcounts) {
    constexpr int NT = 16 * T;
    constexpr int B = 128 / T;                 // samples per batch: NT x B = 2048 values per LDS array
    constexpr int STRIDE = B + 2;              // == 2 (mod 32): the fragment reads hit distinct bank pairs
    constexpr int NSL = 4 / T;                 // waves sharing a tile row split the batch's k-steps
    constexpr int NG = xcov_ng(PAIR, VAR);
    constexpr int RPP = 256 / B;               // component rows per load pass
    constexpr int NP = NT / RPP;               // load passes (8)
    constexpr int XCOV_UNROLL = (T == 4 && PAIR && VAR) ? 1 : 8;
    __shared__ double lf[NT * STRIDE];
    __shared__ double lc[PAIR ? NT * STRIDE : 1];
    __shared__ double lfb[NT * STRIDE];
    __shared__ double lcb[PAIR ? NT * STRIDE : 1];
    __shared__ int keep_s[B];
    __shared__ int ldc[4][2];
    __shared__ double sh_a[NT], sh_b[NT];

    int bi, bj;
    xcov_block(blockIdx.y, NB, bi, bj);
    const bool diag = bi == bj;
    const int ra = bi * NT, rb = bj * NT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int I = wave % T, kslice = wave / T;

    // load role: sample ls of the batch, component rows lr + q RPP of the row (a) and column (b) window; shifts from LDS
    const int ls = threadIdx.x % B, lr = threadIdx.x / B;
    if (threadIdx.x < NT) {
        sh_a[threadIdx.x] = ra + (int)threadIdx.x < M ? shift[ra + threadIdx.x] : 0.0;
        sh_b[threadIdx.x] = rb + (int)threadIdx.x < M ? shift[rb + threadIdx.x] : 0.0;
    }
    const int na = M - ra, nb = diag ? 0 : M - rb;   // rows of the windows inside the matrix
    double pf[NP][4];
    auto load = [&](int64_t b) {
        const int64_t idx = b * B + ls;
        const bool v = idx < n;
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const int row = lr + q * RPP;
            const int64_t oa = (int64_t)(ra + row) * n + idx, ob = (int64_t)(rb + row) * n + idx;
            pf[q][0] = (v && row < na) ? fine[oa] : 0.0;
            pf[q][1] = (PAIR && v && row < na) ? coarse[oa] : 0.0;
            pf[q][2] = (v && row < nb) ? fine[ob] : 0.0;
            pf[q][3] = (PAIR && v && row < nb) ? coarse[ob] : 0.0;
        }
    };

    v4f64 acc[NG][T];
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int j = 0; j < T; ++j) acc[g][j] = (v4f64){0.0, 0.0, 0.0, 0.0};
    int n_keep = 0, n_rm = 0;

    const int64_t n_batches = (n + B - 1) / B;
    int64_t batch = blockIdx.x;
    if (batch < n_batches) load(batch);
    for (; batch < n_batches; batch += gridDim.x) {
        // ---- keep flags of the batch ----
        if (threadIdx.x < B) {
            const int64_t idx = batch * B + threadIdx.x;
            keep_s[threadIdx.x] = (idx < n && (!mask || mask[idx] != 0)) ? 1 : 0;
        }
        __syncthreads();
        if (!mask) {   // one block holds every component (host: NB == 1): a NaN anywhere in the sample drops it
            bool bad = false;
#pragma unroll
            for (int q = 0; q < NP; ++q) bad = bad || (pf[q][0] != pf[q][0]) || (PAIR && pf[q][1] != pf[q][1]);
            if (bad) keep_s[ls] = 0;
            __syncthreads();
        }
        if (blockIdx.y == 0 && threadIdx.x < B) {
            const int64_t idx = batch * B + threadIdx.x;
            const int k = keep_s[threadIdx.x];
            n_keep += k;
            n_rm += (int)(idx < n && !k);
        }
        // ---- shifted, masked values -> LDS ----
        const bool k = keep_s[ls] != 0;
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const int row = lr + q * RPP;
            const int o = row * STRIDE + ls;
            const double sa = sh_a[row];
            lf[o] = k ? pf[q][0] - sa : 0.0;          // (rows outside the matrix: 0 - 0)
            if (PAIR) lc[o] = k ? pf[q][1] - sa : 0.0;
            if (!diag) {
                const double sb = sh_b[row];
                lfb[o] = k ? pf[q][2] - sb : 0.0;
                if (PAIR) lcb[o] = k ? pf[q][3] - sb : 0.0;
            }
        }
        if (batch + gridDim.x < n_batches) load(batch + gridDim.x);     // in flight during the matrix phase
        __syncthreads();
        // ---- matrix phase ----
        const double *__restrict__ fB = diag ? lf : lfb;
        const double *__restrict__ cB = diag ? lc : lcb;
        const int arow = 16 * I + (lane & 15);
        // (the heaviest form -- 20 MFMAs per k-step, 96 accumulator registers -- is not unrolled: the hoisted LDS reads of later
        // k-steps would not fit the 256 registers of two workgroups per CU and spilled)
#pragma unroll XCOV_UNROLL
        for (int kk = 0; kk < B / 4 / NSL; ++kk) {
            const int col = 4 * (kslice + kk * NSL) + (lane >> 4);
            const double fa = lf[arow * STRIDE + col];
            double da = fa, sa = fa;
            if (PAIR) {
                const double ca = lc[arow * STRIDE + col];
                da = fa - ca;
                sa = fa + ca;
            }
#pragma unroll
            for (int J = 0; J < T; ++J) {
                const int brow = 16 * J + (lane & 15);
                const double fb = fB[brow * STRIDE + col];
                if (PAIR) {
                    const double cb = cB[brow * STRIDE + col];
                    const double db = fb - cb, sb = fb + cb;
                    acc[0][J] = __builtin_amdgcn_mfma_f64_16x16x4f64(da, sb, acc[0][J], 0, 0, 0);
                    acc[0][J] = __builtin_amdgcn_mfma_f64_16x16x4f64(sa, db, acc[0][J], 0, 0, 0);
                    if (VAR) {
                        acc[1][J] = __builtin_amdgcn_mfma_f64_16x16x4f64(da * da, sb * sb, acc[1][J], 0, 0, 0);
                        acc[1][J] = __builtin_amdgcn_mfma_f64_16x16x4f64(sa * sa, db * db, acc[1][J], 0, 0, 0);
                        acc[NG - 1][J] = __builtin_amdgcn_mfma_f64_16x16x4f64(da * sa, db * sb, acc[NG - 1][J], 0, 0, 0);
                    }
                } else {
                    acc[0][J] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa, fb, acc[0][J], 0, 0, 0);
                    if (VAR) acc[NG - 1][J] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa * fa, fb * fb, acc[NG - 1][J], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // ---- partial block of this workgroup (one row per k-slice) ----
    // f64 MFMA C/D layout: register r of lane l holds (row l / 16 + 4 r, column l % 16) of the tile
    double *__restrict__ prow = partials + (((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * NSL + kslice) * (NG * NT * NT);
#pragma unroll
    for (int J = 0; J < T; ++J)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * I + (lane >> 4) + 4 * r, col = 16 * J + (lane & 15);
#pragma unroll
            for (int g = 0; g < NG; ++g) prow[g * NT * NT + row * NT + col] = acc[g][J][r];
        }
    if (blockIdx.y == 0) {
        n_keep = wave_sum_i(n_keep);
        n_rm = wave_sum_i(n_rm);
        if (lane == 0) { ldc[wave][0] = n_keep; ldc[wave][1] = n_rm; }
        __syncthreads();
        if (threadIdx.x < 2)
            pcounts[(int64_t)blockIdx.x * 2 + threadIdx.x] = ldc[0][threadIdx.x] + ldc[1][threadIdx.x] + ldc[2][threadIdx.x] + ldc[3][threadIdx.x];
    }
}

// Level totals += the partial rows of one launch, fixed order: 16 entries per workgroup, 64 row groups summed through LDS.
// grid (ceil(NT^2 / 16) [+ 1: the sample counts], block pairs), 1024 threads.  Upper entries only; each is added to (R, C) and
// to its mirror (C, R) with the same value, so the totals stay bitwise symmetric.
__global__ __launch_bounds__(1024) void k_xcov_reduce(const double *__restrict__ partials, int nrows, int NT, int NG, int M, int NB,
                                                      int pair, int var, double *__restrict__ tot_s, double *__restrict__ tot_sp,
                                                      const int64_t *__restrict__ pcounts, int nslices,
                                                      int64_t *__restrict__ counts) {
    __shared__ double lds[3][64][17];
    const int c = threadIdx.x & 15, g = threadIdx.x >> 4;
    if (pcounts && blockIdx.x == gridDim.x - 1) {
        if (blockIdx.y == 0 && threadIdx.x < 64) {
            int64_t a = 0, b = 0;
            for (int i = threadIdx.x; i < nslices; i += 64) { a += pcounts[2 * i]; b += pcounts[2 * i + 1]; }
            for (int off = 32; off >= 1; off >>= 1) { a += __shfl_xor(a, off, 64); b += __shfl_xor(b, off, 64); }
            if (threadIdx.x == 0) { counts[0] += a; counts[1] += b; }
        }
        return;
    }
    const int NN = NT * NT;
    const int e = blockIdx.x * 16 + c;
    const double *__restrict__ base = partials + (int64_t)blockIdx.y * nrows * NG * NN;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    if (e < NN)
        for (int q = g; q < nrows; q += 64) {
            const double *row = base + (int64_t)q * NG * NN;
            a0 += row[e];
            if (NG > 1) a1 += row[NN + e];
            if (NG > 2) a2 += row[2 * NN + e];
        }
    lds[0][g][c] = a0;
    lds[1][g][c] = a1;
    lds[2][g][c] = a2;
    __syncthreads();
    if (g != 0 || e >= NN) return;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0;
#pragma unroll 8
    for (int k = 0; k < 64; ++k) {
        v0 += lds[0][k][c];
        v1 += lds[1][k][c];
        v2 += lds[2][k][c];
    }
    int bi, bj;
    xcov_block(blockIdx.y, NB, bi, bj);
    const int r = e / NT, cc = e % NT;
    if (bi == bj && r > cc) return;                // lower half of a diagonal block: its mirror is written below
    const int R = bi * NT + r, C = bj * NT + cc;
    if (R >= M || C >= M) return;
    const double s = pair ? 0.5 * v0 : v0;
    const int64_t u = (int64_t)R * M + C, l = (int64_t)C * M + R;
    tot_s[u] += s;
    if (u != l) tot_s[l] += s;
    if (var) {
        const double sp = pair ? 0.25 * (v1 + 2.0 * v2) : v1;
        tot_sp[u] += sp;
        if (u != l) tot_sp[l] += sp;
    }
}

// totals [L][2][M * M] + counts [L][2] -> the accumulator's output block (n | n_rm | n, n_rm as fp64 | s | sp)
__global__ void k_xcov_finalize(const double *__restrict__ totals, const int64_t *__restrict__ counts, int L, int64_t MM,
                                int mean_only, int64_t *__restrict__ out_n, double *__restrict__ out_nd, double *__restrict__ out_s,
                                double *__restrict__ out_sp) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    if (tid < L) {
        out_n[tid] = counts[2 * tid];
        out_n[L + tid] = counts[2 * tid + 1];
        out_nd[tid] = (double)counts[2 * tid];
        out_nd[L + tid] = (double)counts[2 * tid + 1];
    }
    for (int64_t i = tid; i < (int64_t)L * MM; i += stride) {
        const int64_t l = i / MM, k = i % MM;
        out_s[i] = totals[(2 * l) * MM + k];
        out_sp[i] = mean_only ? __builtin_nan("") : totals[(2 * l + 1) * MM + k];
    }
}

template <int T, bool PAIR, bool VAR>
static void xcov_launch_t(dim3 grid, const double *d_f, const double *d_c, const uint8_t *mask, const double *shift, int64_t n, int M,
                          int NB, double *partials, int64_t *pcounts) {
    hipLaunchKernelGGL((k_xcov_accum<T, PAIR, VAR>), grid, dim3(256), 0, rt().stream, d_f, d_c, mask, shift, n, M, NB, partials, pcounts);
}

template <int T>
static void xcov_launch(bool pair, bool var, dim3 grid, const double *d_f, const double *d_c, const uint8_t *mask, const double *shift,
                        int64_t n, int M, int NB, double *partials, int64_t *pcounts) {
    if (pair && var) xcov_launch_t<T, true, true>(grid, d_f, d_c, mask, shift, n, M, NB, partials, pcounts);
    else if (pair) xcov_launch_t<T, true, false>(grid, d_f, d_c, mask, shift, n, M, NB, partials, pcounts);
    else if (var) xcov_launch_t<T, false, true>(grid, d_f, d_c, mask, shift, n, M, NB, partials, pcounts);
    else xcov_launch_t<T, false, false>(grid, d_f, d_c, mask, shift, n, M, NB, partials, pcounts);
}

// One chunk [M][n] (device pointers) of level `level` into the totals: [mask pass] + one accumulation launch + one reduction.
int launch_xcov_push(mlmc_accum *a, int level, const double *d_f, const double *d_c, int64_t n) {
    if (n == 0) return 0;
    const int M = a->n_comp;
    const int T = xcov_T(M), NT = 16 * T, NSL = 4 / T, B = 128 / T;
    const int NB = (M + NT - 1) / NT, NBP = NB * (NB + 1) / 2;
    const bool pair = d_c != nullptr, var = !a->mean_only;
    const int NG = xcov_ng(pair, var);
    const int64_t n_batches = (n + B - 1) / B;
    const size_t per_slice = (size_t)NBP * NSL * NG * NT * NT * sizeof(double);
    // slices: about two workgroups per CU over all block pairs, at least four batches each, partial rows within the scratch bound
    int64_t ns = (2 * (int64_t)rt().n_cu + NBP - 1) / NBP;
    ns = std::min<int64_t>(ns, (n_batches + 3) / 4);
    ns = std::min<int64_t>(ns, (int64_t)(XCOV_SCRATCH_BYTES / per_slice));
    if (ns < 1) ns = 1;
    if (int rc = ensure((void **)&a->d_partials, &a->partials_cap, per_slice * (size_t)ns)) return rc;
    if (int rc = ensure((void **)&a->d_pcounts, &a->pcounts_cap, sizeof(int64_t) * 2 * (size_t)ns)) return rc;
    const uint8_t *mask = nullptr;
    if (NB > 1) if (int rc = ensure((void **)&a->d_mask, &a->mask_cap, (size_t)n)) return rc;
    hipStream_t st = rt().stream;
    if (int rc = timing_begin(a)) return rc;
    if (NB > 1) {
        const int64_t want = (n + 255) / 256;
        hipLaunchKernelGGL(k_xcov_mask, dim3((unsigned)std::min<int64_t>(want, 4096)), dim3(256), 0, st, d_f, d_c, n, M, a->d_mask);
        MLMC_HIP_CHECK(hipGetLastError());
        mask = a->d_mask;
    }
    const dim3 grid((unsigned)ns, (unsigned)NBP);
    if (T == 1) xcov_launch<1>(pair, var, grid, d_f, d_c, mask, a->d_shift, n, M, NB, a->d_partials, a->d_pcounts);
    else if (T == 2) xcov_launch<2>(pair, var, grid, d_f, d_c, mask, a->d_shift, n, M, NB, a->d_partials, a->d_pcounts);
    else xcov_launch<4>(pair, var, grid, d_f, d_c, mask, a->d_shift, n, M, NB, a->d_partials, a->d_pcounts);
    MLMC_HIP_CHECK(hipGetLastError());
    const int64_t MM = (int64_t)M * M;
    double *tot_s = a->d_totals + (int64_t)level * 2 * MM;
    hipLaunchKernelGGL(k_xcov_reduce, dim3((unsigned)((NT * NT + 15) / 16 + 1), (unsigned)NBP), dim3(1024), 0, st, a->d_partials,
                       (int)(ns * NSL), NT, NG, M, NB, pair ? 1 : 0, var ? 1 : 0, tot_s, tot_s + MM, a->d_pcounts, (int)ns,
                       a->d_counts + 2 * (int64_t)level);
    MLMC_HIP_CHECK(hipGetLastError());
    if (int rc = timing_end(a)) return rc;
    a->launches += 1;
    a->alg_bytes += (int64_t)n * (pair ? 16 : 8) * M;
    const int mfma_per_tile = pair ? (var ? 5 : 2) : (var ? 2 : 1);
    a->mfma_flops += (int64_t)512 * NBP * T * T * mfma_per_tile * n;
    return 0;
}

int launch_xcov_finalize(mlmc_accum *a) {
    const int64_t MM = (int64_t)a->n_comp * a->n_comp;
    const int64_t total = (int64_t)a->n_levels * MM;
    const int64_t want = (std::max<int64_t>(total, a->n_levels) + 255) / 256;
    hipLaunchKernelGGL(k_xcov_finalize, dim3((unsigned)std::min<int64_t>(want, 8192)), dim3(256), 0, rt().stream, a->d_totals, a->d_counts,
                       a->n_levels, MM, a->mean_only ? 1 : 0, a->d_out_n, a->d_out_nd, a->d_out_s, a->d_out_sp);
    MLMC_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace mlmc
