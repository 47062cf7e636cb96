// The Gaussian copula of mlmc_density_sample_joint_batch / mlmc_density_sample_conditional_batch on the device (gfx950): seeded
// latent normals and the copula uniforms u = clamp(normcdf(F z)) (conditional: of shift + F z) that k_q_sample (density.hip) then
// inverts.  The host path of both entries is density.hip's (q_copula).
//
//   k_cop_normals  : Z[k][c] = normcdfinv(uniform of (seed, streams[k], first + c)), negated for the odd draws of an antithetic
//                    call; one thread per element, consecutive lanes write consecutive draws
//   k_cop_uniforms : U = clamp(normcdf(F Z)) as an fp64 GEMM on the matrix cores (v_mfma_f64_16x16x4_f64) with the epilogue on the
//                    accumulators.  One workgroup of 4 waves owns a tile of 64 rows x 64 draws; wave w owns rows 16 w .. 16 w + 15 of
//                    it and all 64 draws (4 accumulator tiles, 16 doubles per lane).  It walks K from 0 in panels of 32: the F panel
//                    [64][32] and the Z panel [32][64] go to LDS with zeros beyond M, K and the draws of the call, then 8 steps of 4 k.
//                    Row tile = blockIdx.y: row tiles beyond the first re-read the same Z panels from memory.
//                    The instance with SHIFT (mlmc_density_sample_conditional_batch) has the set on blockIdx.z: every set forms the
//                    product of its tile anew and adds its own shift in the epilogue.  The instances with
//                    TSCALE (the Student-t copula) store y itself for k_tcop_map (copula_t.hip).
// Neither kernel loops over rows: the compiler would keep the constants of the inlined normcdfinv / normcdf in registers across
// the loop (256 and 208 VGPRs instead of 24 and 114).
// y[m][c] is the chain acc = mfma(F[m][4 s .. 4 s + 3], Z[4 s .. 4 s + 3][c], acc), s = 0, 1, ... from acc = 0: what it adds and in
// which order depends on row m of F and column c of Z alone, not on the tile the element sits in, on the other rows or on the
// launch.  A padded k adds F = 0 times a finite z: an exact zero.
#include <algorithm>

#include "copula.hpp"

namespace mlmc {

typedef double v4f64 __attribute__((ext_vector_type(4)));

constexpr int COP_NORMAL_THREADS = 256;
constexpr int COP_TILE = 64;                           // rows and draws of a workgroup's tile
constexpr int COP_PANEL = 32;                          // k per LDS panel
constexpr int COP_THREADS = 256;
constexpr int COP_F_STRIDE = COP_PANEL + 1;            // odd: the 16 rows an A operand reads fall into different banks
constexpr int COP_Z_STRIDE = COP_TILE + 8;             // the 4 k a B operand reads are 8 doubles apart in the banks

__global__ __launch_bounds__(COP_NORMAL_THREADS) void k_cop_normals(uint64_t seed, const uint32_t *__restrict__ streams,
                                                                     int64_t first, int64_t ncols, int antithetic,
                                                                     double *__restrict__ Z, int64_t ldz) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncols) return;
    const uint64_t j = (uint64_t)(first + c);
    const int k = blockIdx.y;
    // an odd multiple of 2^-53 in (0, 1): z is finite
    const double z = normcdfinv(q_uniform(seed, streams[k], antithetic ? j >> 1 : j));
    Z[(int64_t)k * ldz + c] = (antithetic && (j & 1)) ? -z : z;
}

// SHIFT (mlmc_density_sample_conditional_batch): set = blockIdx.z; the epilogue adds shift[set * set_rows + row] to the finished
// chain, one rounded addition, and the tile goes to rows set * set_rows + row of U.  A lane's four rows are its registers' rows for
// every J, so it loads its four shifts once, ahead of the panels, and the epilogue waits for no memory.
// TSCALE (mlmc_density_sample_joint_t_batch): `mix` is the mixing scale s [ncols] of the draws; the epilogue multiplies the
// finished chain by s[column], one rounded multiplication, and stores y itself: k_tcop_map (copula_t.hip) maps it in place.
// SHIFT and TSCALE (mlmc_density_sample_conditional_t_batch): set = blockIdx.z as under SHIFT; a lane loads its four shifts and
// its set's scale once, ahead of the panels, and the epilogue stores y = shift (+) ((acc (x) s[column]) (x) scale[set]): three
// rounded operations in this order, so that scale = 1 and shift = 0 leave the bits of the TSCALE instance's y (up to the sign
// of a zero, which the map does not see).  k_tcop_map maps the rows of all sets in place.
template <bool SHIFT, bool TSCALE = false>
__global__ __launch_bounds__(COP_THREADS) void k_cop_uniforms(const double *__restrict__ F, int M, int K, const double *__restrict__ Z,
                                                              int64_t ldz, int64_t ncols, double *__restrict__ U, int64_t ldu,
                                                              const double *__restrict__ shift, int64_t set_rows,
                                                              const double *__restrict__ mix, const double *__restrict__ set_scale) {
    __shared__ double fl[COP_TILE * COP_F_STRIDE];
    __shared__ double zl[COP_PANEL * COP_Z_STRIDE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t col0 = (int64_t)blockIdx.x * COP_TILE;
    const int row0 = blockIdx.y * COP_TILE;
    [[maybe_unused]] double sh[4] = {0.0, 0.0, 0.0, 0.0};
    if constexpr (SHIFT) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + 16 * wave + (lane >> 4) + 4 * r;
            if (row < M) sh[r] = shift[(int64_t)blockIdx.z * set_rows + row];
        }
    }
    [[maybe_unused]] double sc = 1.0;
    if constexpr (SHIFT && TSCALE) sc = set_scale[blockIdx.z];
    v4f64 acc[COP_TILE / 16];
#pragma unroll
    for (int J = 0; J < COP_TILE / 16; ++J) acc[J] = (v4f64){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += COP_PANEL) {
        __syncthreads();                               // the previous panel has been read
#pragma unroll
        for (int i = 0; i < COP_TILE * COP_PANEL / COP_THREADS; ++i) {
            const int idx = threadIdx.x + i * COP_THREADS;
            const int r = idx / COP_PANEL, kc = idx % COP_PANEL;
            const int row = row0 + r, k = k0 + kc;
            fl[r * COP_F_STRIDE + kc] = (row < M && k < K) ? F[(int64_t)row * K + k] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < COP_PANEL * COP_TILE / COP_THREADS; ++i) {
            const int idx = threadIdx.x + i * COP_THREADS;
            const int kr = idx / COP_TILE, c = idx % COP_TILE;
            const int k = k0 + kr;
            const int64_t col = col0 + c;
            zl[kr * COP_Z_STRIDE + c] = (k < K && col < ncols) ? Z[(int64_t)k * ldz + col] : 0.0;
        }
        __syncthreads();
        // A operand: lane l holds F[row l & 15][k = l >> 4]; B operand: Z[k = l >> 4][column l & 15]
#pragma unroll
        for (int s = 0; s < COP_PANEL / 4; ++s) {
            const int kk = 4 * s + (lane >> 4);
            const double a = fl[(16 * wave + (lane & 15)) * COP_F_STRIDE + kk];
#pragma unroll
            for (int J = 0; J < COP_TILE / 16; ++J) {
                const double b = zl[kk * COP_Z_STRIDE + 16 * J + (lane & 15)];
                acc[J] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[J], 0, 0, 0);
            }
        }
    }
    // f64 MFMA C/D layout: register r of lane l holds (row l / 16 + 4 r, column l % 16) of the tile
#pragma unroll
    for (int J = 0; J < COP_TILE / 16; ++J)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + 16 * wave + (lane >> 4) + 4 * r;
            const int64_t col = col0 + 16 * J + (lane & 15);
            if constexpr (SHIFT && TSCALE) {
                if (row < M && col < ncols)
                    U[((int64_t)blockIdx.z * set_rows + row) * ldu + col] =
                        __dadd_rn(sh[r], __dmul_rn(__dmul_rn(acc[J][r], mix[col]), sc));
            } else if constexpr (SHIFT) {
                if (row < M && col < ncols)
                    U[((int64_t)blockIdx.z * set_rows + row) * ldu + col] =
                        fmin(fmax(normcdf(__dadd_rn(sh[r], acc[J][r])), 0x1p-53), 1.0 - 0x1p-53);
            } else if constexpr (TSCALE) {
                if (row < M && col < ncols) U[(int64_t)row * ldu + col] = __dmul_rn(acc[J][r], mix[col]);
            } else {
                if (row < M && col < ncols) U[(int64_t)row * ldu + col] = fmin(fmax(normcdf(acc[J][r]), 0x1p-53), 1.0 - 0x1p-53);
            }
        }
}

void cop_launch_normals(hipStream_t st, uint64_t seed, const uint32_t *streams, int K, int64_t first, int64_t ncols, int antithetic,
                        double *Z, int64_t ldz) {
    // one thread per element, row k of a launch = blockIdx.y: more rows than a grid has in y go in several launches
    for (int k0 = 0; k0 < K; k0 += 65535) {
        const dim3 grid((unsigned)((ncols + COP_NORMAL_THREADS - 1) / COP_NORMAL_THREADS), (unsigned)std::min(K - k0, 65535));
        hipLaunchKernelGGL(k_cop_normals, grid, dim3(COP_NORMAL_THREADS), 0, st, seed, streams + k0, first, ncols, antithetic,
                           Z + (int64_t)k0 * ldz, ldz);
    }
}

void cop_launch_uniforms(hipStream_t st, const double *F, int M, int K, const double *Z, int64_t ldz, int64_t ncols, double *U,
                         int64_t ldu) {
    // row tile of a launch = blockIdx.y: more tiles than a grid has in y go in several launches
    constexpr int rows = 65535 * COP_TILE;
    for (int m0 = 0; m0 < M; m0 += rows) {
        const int Ml = std::min(M - m0, rows);
        const dim3 grid((unsigned)((ncols + COP_TILE - 1) / COP_TILE), (unsigned)((Ml + COP_TILE - 1) / COP_TILE));
        hipLaunchKernelGGL(k_cop_uniforms<false>, grid, dim3(COP_THREADS), 0, st, F + (int64_t)m0 * K, Ml, K, Z, ldz, ncols,
                           U + (int64_t)m0 * ldu, ldu, (const double *)nullptr, (int64_t)0, (const double *)nullptr, (const double *)nullptr);
    }
}

void cop_launch_scaled_product(hipStream_t st, const double *F, int M, int K, const double *Z, int64_t ldz, int64_t ncols, double *U,
                               int64_t ldu, const double *s) {
    constexpr int rows = 65535 * COP_TILE;
    for (int m0 = 0; m0 < M; m0 += rows) {
        const int Ml = std::min(M - m0, rows);
        const dim3 grid((unsigned)((ncols + COP_TILE - 1) / COP_TILE), (unsigned)((Ml + COP_TILE - 1) / COP_TILE));
        hipLaunchKernelGGL((k_cop_uniforms<false, true>), grid, dim3(COP_THREADS), 0, st, F + (int64_t)m0 * K, Ml, K, Z, ldz, ncols,
                           U + (int64_t)m0 * ldu, ldu, (const double *)nullptr, (int64_t)0, s, (const double *)nullptr);
    }
}

void cop_launch_uniforms_shifted(hipStream_t st, const double *F, int M, int K, const double *Z, int64_t ldz, int64_t ncols, double *U,
                                 int64_t ldu, const double *shift, int B, int64_t set_rows) {
    // set of a launch = blockIdx.z, row tile = blockIdx.y: more of either than a grid has go in several launches
    constexpr int rows = 65535 * COP_TILE;
    for (int b0 = 0; b0 < B; b0 += 65535)
        for (int m0 = 0; m0 < M; m0 += rows) {
            const int Ml = std::min(M - m0, rows);
            const dim3 grid((unsigned)((ncols + COP_TILE - 1) / COP_TILE), (unsigned)((Ml + COP_TILE - 1) / COP_TILE),
                            (unsigned)std::min(B - b0, 65535));
            hipLaunchKernelGGL(k_cop_uniforms<true>, grid, dim3(COP_THREADS), 0, st, F + (int64_t)m0 * K, Ml, K, Z, ldz, ncols,
                               U + ((int64_t)b0 * set_rows + m0) * ldu, ldu, shift + (int64_t)b0 * set_rows + m0, set_rows,
                               (const double *)nullptr, (const double *)nullptr);
        }
}

void cop_launch_scaled_shifted(hipStream_t st, const double *F, int M, int K, const double *Z, int64_t ldz, int64_t ncols, double *U,
                               int64_t ldu, const double *shift, const double *s, const double *scale, int B, int64_t set_rows) {
    // the split of cop_launch_uniforms_shifted
    constexpr int rows = 65535 * COP_TILE;
    for (int b0 = 0; b0 < B; b0 += 65535)
        for (int m0 = 0; m0 < M; m0 += rows) {
            const int Ml = std::min(M - m0, rows);
            const dim3 grid((unsigned)((ncols + COP_TILE - 1) / COP_TILE), (unsigned)((Ml + COP_TILE - 1) / COP_TILE),
                            (unsigned)std::min(B - b0, 65535));
            hipLaunchKernelGGL((k_cop_uniforms<true, true>), grid, dim3(COP_THREADS), 0, st, F + (int64_t)m0 * K, Ml, K, Z, ldz, ncols,
                               U + ((int64_t)b0 * set_rows + m0) * ldu, ldu, shift + (int64_t)b0 * set_rows + m0, set_rows, s, scale + b0);
        }
}

}  // namespace mlmc
