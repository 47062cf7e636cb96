// Batched maximum-entropy densities on the device (gfx950): B independent problems of SimpleDistribution's functional
// (mlmc/tool/simple_distribution.py:50-94,198-327), one per scalar component of a vector quantity.
//
// k_me_coop (maxent.hip) spreads ONE small problem over up to 128 workgroups that meet at a grid barrier several times per
// Newton step; it is bound by that barrier's latency and needs the grid co-resident.  Here one workgroup owns one problem
// for the whole solve: no grid barrier, no co-residency requirement, B may exceed the CU count (the problems queue as
// workgroups), and every reduction inside a workgroup has a fixed order, so a problem's result does not depend on the batch
// it is in or on its position there.
//
//   k_meb_phi   : Phi_b[q][i] = phi_i(x_q) / sigma_i of every problem, one launch (grid: problem x 32-point block); the
//                 quadrature nodes are formed on the device with the host's formula (same roundings: -ffp-contract=off)
//   k_meb_solve : the damped Newton iteration of k_me_coop, one 256-thread workgroup per problem.  Phi_b does not fit in LDS
//                 (Q x R1 x 8 B = 527 KB at Q = 1344, R1 = 49), so every pass streams it from L2 / MALL in QS-row tiles; the
//                 tile and the L D L^T matrix share (alias) LDS, as psi and Lm do in k_me_coop.  Per tile: rho w of the rows
//                 (8 lanes per row), the gradient (one lane per moment) and the Hessian Phi^T diag(rho w) Phi in 4 x 4
//                 register blocks of the upper triangle (plain fp64 FMA; the accumulators live in VGPRs across the tiles).
// Algorithm and constants as k_me_coop without penalties: speculative full step, Armijo backtracking four step lengths per
// pass, tau schedule 1e-10 (1 + |F|) / 1e-8 (1 + |F|), x100 on failure, x0.1 after a full step, convergence on ||g||_2.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "device_basis.hpp"
#include "maxent_batch.hpp"

namespace mlmc {

constexpr int MEB_THREADS = 256;
constexpr int MEB_MAX_R = 128;        // moments per problem (R1)
constexpr int MEB_MAX_BASE = 512;     // underlying terms of a transformed basis (LDS of k_meb_phi: 32 x 513 doubles)
constexpr int MEB_EVAL_PTS = 32;      // quadrature points per workgroup of k_meb_phi
constexpr int MEB_NS_MAX = 3;         // 4 x 4 Hessian blocks per thread: ceil(32 * 33 / 2 / 256) at R1 = 128
constexpr int MEB_LDS_LIMIT = 160 * 1024;

struct MebProb {
    BasisParams bp;
    const double *scale;     // device scale_c [bp.size] (Legendre: P_i = scale_c[i] q_i)
    const double *matrix;    // device [out_size][bp.size] of a TransformedMoments basis, or nullptr
    int n_terms;             // terms generated per point: bp.size with a matrix, else R1
    int R1;
    int64_t phi_off;         // Phi_b = phi + phi_off, [Q][R1]
    double a, b;             // integration domain
};

// quadrature node / weight q of the composite rule on [a, b] -- the same expressions as the host's (mlmc_maxent_solve)
__device__ __forceinline__ void meb_node(double a, double b, int nint, int deg, const double *gx, const double *gw, int q,
                                         double &x, double &w) {
    const int k = q / deg, j = q - k * deg;
    const double h = (b - a) / nint;
    const double lo = a + k * h, hi = (k == nint - 1) ? b : a + (k + 1) * h;
    x = (gx[j] + 1.0) / 2.0 * (hi - lo) + lo;      // simple_distribution.py:227
    w = gw[j] * (hi - lo) / 2.0;                   // :228
}

template <int KIND>
__device__ void meb_terms(const BasisParams &bp, const double *scale, double x, int n, double *out) {
    bool keep;
    const double t = transform_value(bp, x, keep);
    TermGen<KIND> g;
    g.init(keep ? t : 0.0, 1.0, bp);
    const double nan = __builtin_nan("");
    for (int r = 0; r < n; ++r) {
        double v = g.next(r);
        if (KIND == MLMC_LEGENDRE) v *= scale[r];
        out[r] = keep ? v : nan;
    }
}

// Phi of every problem: grid (B, ceil(Q / 32)); the underlying terms of 32 points go to LDS, then the transform rows
// (sequential sums over r, as k_apply_matrix) and the division by sigma (as k_me_scale_cols).
__global__ __launch_bounds__(MEB_THREADS) void k_meb_phi(const MebProb *__restrict__ probs, const double *__restrict__ sigma, int ldv,
                                                         const double *__restrict__ gx, const double *__restrict__ gw, int nint,
                                                         int deg, double *__restrict__ phi) {
    extern __shared__ double sm[];
    const MebProb P = probs[blockIdx.x];
    const int Q = nint * deg, nt = P.n_terms, ldt = nt + 1, R1 = P.R1;
    const int q0 = blockIdx.y * MEB_EVAL_PTS;
    if (q0 >= Q) return;
    const int np = min(MEB_EVAL_PTS, Q - q0);
    const double *sig = sigma + (int64_t)blockIdx.x * ldv;
    if ((int)threadIdx.x < np) {
        double x, w;
        meb_node(P.a, P.b, nint, deg, gx, gw, q0 + threadIdx.x, x, w);
        double *row = sm + threadIdx.x * ldt;
        switch (P.bp.kind) {
            case MLMC_LEGENDRE: meb_terms<MLMC_LEGENDRE>(P.bp, P.scale, x, nt, row); break;
            case MLMC_MONOMIAL: meb_terms<MLMC_MONOMIAL>(P.bp, P.scale, x, nt, row); break;
            case MLMC_FOURIER: meb_terms<MLMC_FOURIER>(P.bp, P.scale, x, nt, row); break;
            default: meb_terms<MLMC_SPLINE>(P.bp, P.scale, x, nt, row); break;
        }
    }
    __syncthreads();
    double *out = phi + P.phi_off + (int64_t)q0 * R1;
    for (int idx = threadIdx.x; idx < np * R1; idx += MEB_THREADS) {
        const int t = idx / R1, j = idx - t * R1;
        const double *row = sm + t * ldt;
        double v;
        if (P.matrix) {
            const double *mr = P.matrix + (int64_t)j * nt;
            v = 0.0;
            for (int r = 0; r < nt; ++r) v = __builtin_fma(row[r], mr[r], v);
        } else {
            v = row[j];
        }
        out[idx] = v / sig[j];
    }
}

struct MebArgs {
    const MebProb *probs;
    const double *phi;
    const double *mus;       // [B][ldv] mu_i / sigma_i
    const double *sigma;     // [B][ldv]
    const double *lam0;      // [B][ldv] start
    const double *gx, *gw;   // Gauss-Legendre rule on [-1, 1]
    double *out;             // [B][ldo]: result[8] | lambda[ldv] | gradient[ldv] | Hessian[ldv][ldv] (want_h)
    int64_t ldo;
    int ldv, nint, deg, QS, max_it, want_h;
    double tol;
};

// compensated (Neumaier) running sum: the integral and the gradient are sums of Q = 1344 terms taken by ONE lane in order.
// Plainly summed, their rounding (~sqrt(Q) ulp, and not the same at lam and at lam + p) exceeds the decrease that the Armijo
// test has to see near the solution (0.5 g.H^-1 g ~ 1e-16 at |g| = 1e-8): the step is refused, tau grows, the iteration
// stalls short of tol.  Compensated, both are good to an ulp, like k_me_coop's sums of per-workgroup partials.
struct MebSum {
    double s = 0.0, c = 0.0;
    __device__ __forceinline__ void add(double x) {
        const double t = s + x;
        c += fabs(s) >= fabs(x) ? (s - t) + x : (x - t) + s;
        s = t;
    }
    __device__ __forceinline__ double value() const { return s + c; }
};

__device__ __forceinline__ double meb_readlane(double v, int lane) {   // lane must be wave-uniform
    const unsigned lo = __builtin_amdgcn_readlane((int)__double2loint(v), lane);
    const unsigned hi = __builtin_amdgcn_readlane((int)__double2hiint(v), lane);
    return __hiloint2double((int)hi, (int)lo);
}

// NS = 4 x 4 blocks of the Hessian per thread: 1 up to R1 = 88 (253 blocks), 2 up to 124, 3 up to 128.  The accumulators of
// the larger forms cost VGPRs (occupancy), so the launch picks the smallest that covers the batch's largest R1.
template <int MEB_NS>
__global__ __launch_bounds__(MEB_THREADS) void k_meb_solve(MebArgs A) {
    extern __shared__ double sm[];
    const int pb = blockIdx.x, tid = threadIdx.x;
    const MebProb P = A.probs[pb];
    const int R1 = P.R1, QS = A.QS, nint = A.nint, deg = A.deg, Q = nint * deg;
    const int T4 = (R1 + 3) / 4, RT = 4 * T4, ld = R1 + 1;
    const int nbp = T4 * (T4 + 1) / 2;
    const int alias = max(QS * RT, R1 * ld);
    double *tile = sm;                         // [QS][RT] rows of Phi_b, zero beyond R1 (phases A and line search)
    double *Lm = sm;                           // [R1][ld] L D L^T of H + tau I (phase C) -- aliases the tile
    double *rw = sm + alias;                   // [4][QS] rho w of the tile (four step lengths in the line search)
    double *wt = rw + 4 * QS;                  // [QS] quadrature weights of the tile
    double *lam = wt + QS;                     // [R1]
    double *trial = lam + R1;                  // [R1] point of the current full pass
    double *g = trial + R1;                    // [R1]
    double *pdir = g + R1;                     // [R1]
    double *y = pdir + R1;                     // [R1] 1 / d_k
    double *mus = y + R1;                      // [R1] mu_i / sigma_i
    double *gsum = mus + R1;                   // [R1] sum_q Phi[q][i] rho_q w_q of the last full pass
    double *red = gsum + R1;                   // [16] 0..4 as k_me_coop; 5: integral of the last full pass; 6..9: line search
    __shared__ int bad_s;
    const double *phi = A.phi + P.phi_off;
    const double sigma0 = A.sigma[(int64_t)pb * A.ldv];
    for (int i = tid; i < R1; i += MEB_THREADS) {
        lam[i] = A.lam0[(int64_t)pb * A.ldv + i];
        mus[i] = A.mus[(int64_t)pb * A.ldv + i];
        pdir[i] = 0.0;
        g[i] = 0.0;
    }
    // the thread's 4 x 4 blocks (bi <= bj) of the upper triangle, row-major block index p = tid + 256 s
    int hbi[MEB_NS], hbj[MEB_NS];
#pragma unroll
    for (int s = 0; s < MEB_NS; ++s) {
        int p = tid + MEB_THREADS * s, bi = 0;
        if (p >= nbp) p = 0;
        while (p >= T4 - bi) { p -= T4 - bi; ++bi; }
        hbi[s] = bi;
        hbj[s] = bi + p;
    }
    double hacc[MEB_NS][16];
    __syncthreads();

    auto load_tile = [&](int q0, int nq) {
        __syncthreads();                                            // the previous tile (or Lm) is no longer read
        const double *src = phi + (int64_t)q0 * R1;
        for (int idx = tid; idx < QS * RT; idx += MEB_THREADS) {
            const int t = idx / RT, c = idx - t * RT;
            tile[idx] = (t < nq && c < R1) ? src[t * R1 + c] : 0.0;
        }
        for (int t = tid; t < QS; t += MEB_THREADS) {
            double x, w = 0.0;
            if (t < nq) meb_node(P.a, P.b, nint, deg, A.gx, A.gw, q0 + t, x, w);
            wt[t] = w;
        }
        __syncthreads();
    };

    // full pass at trial = lam + alpha pdir: integral (red[5]), gsum, Hessian blocks (hacc)
    auto pass_full = [&](double alpha) {
        for (int i = tid; i < R1; i += MEB_THREADS) trial[i] = __builtin_fma(alpha, pdir[i], lam[i]);
#pragma unroll
        for (int s = 0; s < MEB_NS; ++s)
#pragma unroll
            for (int e = 0; e < 16; ++e) hacc[s][e] = 0.0;
        MebSum gacc, iacc;
        for (int q0 = 0; q0 < Q; q0 += QS) {
            const int nq = min(QS, Q - q0);
            load_tile(q0, nq);
            for (int item = tid >> 3; item < QS; item += MEB_THREADS / 8) {
                const int sub = tid & 7;
                double power = 0.0;
                for (int i = sub; i < R1; i += 8) power = __builtin_fma(tile[item * RT + i], trial[i], power);
                power += __shfl_xor(power, 1, 64);
                power += __shfl_xor(power, 2, 64);
                power += __shfl_xor(power, 4, 64);
                if (sub == 0) rw[item] = wt[item] * exp(fmin(fmax(-power, -200.0), 200.0));   // simple_distribution.py:256
            }
            __syncthreads();
            if (tid < R1)
                for (int t = 0; t < nq; ++t) gacc.add(tile[t * RT + tid] * rw[t]);
            if (tid == MEB_THREADS - 1)
                for (int t = 0; t < nq; ++t) iacc.add(rw[t]);
#pragma unroll
            for (int s = 0; s < MEB_NS; ++s) {
                if (tid + MEB_THREADS * s < nbp) {
                    const double *ra = tile + 4 * hbi[s], *rb = tile + 4 * hbj[s];
                    for (int t = 0; t < nq; ++t) {
                        const double r = rw[t];
                        double av[4], bv[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) { av[k] = ra[t * RT + k] * r; bv[k] = rb[t * RT + k]; }
#pragma unroll
                        for (int k = 0; k < 4; ++k)
#pragma unroll
                            for (int l = 0; l < 4; ++l) hacc[s][4 * k + l] = __builtin_fma(av[k], bv[l], hacc[s][4 * k + l]);
                    }
                }
            }
        }
        __syncthreads();
        if (tid < R1) gsum[tid] = gacc.value();
        if (tid == MEB_THREADS - 1) red[5] = iacc.value();
        __syncthreads();
    };

    // integrals at lam + (alpha0 / 2^k) pdir, k < 4 -> red[6 + k]
    auto pass_ls = [&](double alpha0) {
        MebSum lacc;
        for (int q0 = 0; q0 < Q; q0 += QS) {
            const int nq = min(QS, Q - q0);
            load_tile(q0, nq);
            for (int item = tid >> 3; item < 4 * QS; item += MEB_THREADS / 8) {
                const int k = item / QS, q = item - k * QS, sub = tid & 7;
                const double alpha = alpha0 / (double)(1 << k);
                double power = 0.0;
                for (int i = sub; i < R1; i += 8) power = __builtin_fma(tile[q * RT + i], __builtin_fma(alpha, pdir[i], lam[i]), power);
                power += __shfl_xor(power, 1, 64);
                power += __shfl_xor(power, 2, 64);
                power += __shfl_xor(power, 4, 64);
                if (sub == 0) rw[k * QS + q] = wt[q] * exp(fmin(fmax(-power, -200.0), 200.0));
            }
            __syncthreads();
            if (tid < 4)
                for (int t = 0; t < nq; ++t) lacc.add(rw[tid * QS + t]);
        }
        __syncthreads();
        if (tid < 4) red[6 + tid] = lacc.value();
        __syncthreads();
    };

    int nit = 0, success = 0;
    double tau = 0.0, F = 0.0, gnorm = 0.0, moment0 = 0.0, gp = 0.0;
    bool spec = false;          // this round's full pass is at lam + pdir (the full Newton step), as in k_me_coop
    bool give_up = false;       // the line search failed at the largest shift: leave after the next phase C (at lam)
    for (int it = 0; it <= A.max_it;) {
        pass_full(spec ? 1.0 : 0.0);
        if (spec) {
            spec = false;
            const double lin0 = F - red[4];                                 // mu~ . lam  (red[4]: integral at lam)
            const double Ft = (lin0 + red[3]) + red[5];
            bool accepted = Ft == Ft && Ft <= F + 1e-4 * gp;
            double alpha = 1.0;
            if (!accepted) {
                alpha = 0.5;                                                // backtracking: alpha / 2^k, four per pass
                for (int batch = 0; batch < 10 && !accepted; ++batch) {
                    pass_ls(alpha);
                    for (int k = 0; k < 4; ++k) {
                        const double ak = alpha / (double)(1 << k);
                        const double Fk = __builtin_fma(ak, red[3], lin0) + red[6 + k];
                        if (Fk == Fk && Fk <= F + 1e-4 * ak * gp) { accepted = true; alpha = ak; break; }
                    }
                    if (!accepted) alpha /= 16.0;
                }
            }
            if (!accepted) {
                tau = (tau == 0.0) ? 1e-8 * (1.0 + fabs(F)) : tau * 100.0;
                // giving up: the sums (hacc, gsum) are those of the rejected trial point -- one more round at lam, so that
                // every output, the Hessian included, belongs to the returned multipliers; phase C then leaves the loop
                if (tau > 1e20) give_up = true;
                continue;                                                   // re-evaluate at lam with the larger shift
            }
            __syncthreads();
            for (int i = tid; i < R1; i += MEB_THREADS) lam[i] = __builtin_fma(alpha, pdir[i], lam[i]);
            __syncthreads();
            tau = (alpha == 1.0) ? tau * 0.1 : tau;
            if (tau < 1e-14) tau = 0.0;
            ++nit;
            if (alpha != 1.0) continue;                                     // the sums are not those of the new lam
        }
        // ---- phase C: gradient, L D L^T of H + tau I, Newton direction ----
        for (int i = tid; i < R1; i += MEB_THREADS) g[i] = mus[i] - gsum[i];
#pragma unroll
        for (int s = 0; s < MEB_NS; ++s) {
            if (tid + MEB_THREADS * s < nbp) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int l = 0; l < 4; ++l) {
                        const int r = 4 * hbi[s] + k, c = 4 * hbj[s] + l;
                        if (r < R1 && c < R1 && (hbi[s] != hbj[s] || k <= l)) {   // upper triangle only: H stays symmetric
                            const double v = hacc[s][4 * k + l] + (r == c ? tau : 0.0);
                            Lm[r * ld + c] = v;
                            Lm[c * ld + r] = v;
                        }
                    }
            }
        }
        if (tid == 0) bad_s = 0;
        __syncthreads();
        {
            double lin = 0.0;
            for (int k = 0; k < R1; ++k) lin = __builtin_fma(mus[k], lam[k], lin);
            F = lin + red[5];
            moment0 = gsum[0] * sigma0;
        }
        // L D L^T in place, one workgroup barrier per column (as k_me_coop): Lm[i][k] = L_ik d_k (i > k), Lm[k][k] = d_k
        for (int k = 0; k < R1; ++k) {
            const double d = Lm[k * ld + k];
            if (!(d > 0.0)) {                       // same value in every thread: uniform exit
                if (tid == 0) bad_s = 1;
                break;
            }
            const double inv_d = 1.0 / d;
            if (tid == 0) y[k] = inv_d;
            for (int i = k + 1 + (tid >> 4); i < R1; i += 16) {
                const double lik = Lm[i * ld + k] * inv_d;
                for (int j = k + 1 + (tid & 15); j <= i; j += 16) Lm[i * ld + j] = __builtin_fma(-lik, Lm[j * ld + k], Lm[i * ld + j]);
            }
            __syncthreads();
        }
        __syncthreads();
        if (tid < 64) {
            // triangular solves by one wave (k_me_coop's column-oriented form): lane j carries entries j and j + 64
            const int j0 = tid, j1 = tid + 64;
            const bool spd = bad_s == 0;
            double v0 = j0 < R1 ? -g[j0] : 0.0, v1 = j1 < R1 ? -g[j1] : 0.0;
            const double id0 = j0 < R1 ? y[j0] : 0.0, id1 = j1 < R1 ? y[j1] : 0.0;
            const int jc0 = j0 < R1 ? j0 : 0, jc1 = j1 < R1 ? j1 : 0;
            const bool two = R1 > 64;
            if (spd) {
                double a0 = Lm[jc0 * ld + 0], a1 = two ? Lm[jc1 * ld + 0] : 0.0, yi = y[0];
                for (int i = 0; i < R1; ++i) {                     // L u = -g, z = D^-1 u
                    const int in = i + 1 < R1 ? i + 1 : i;
                    const double n0 = Lm[jc0 * ld + in], n1 = two ? Lm[jc1 * ld + in] : 0.0, yn = y[in];
                    const double zi = meb_readlane(i < 64 ? v0 : v1, i & 63) * yi;
                    if (j0 == i) v0 = zi;
                    if (j1 == i) v1 = zi;
                    if (j0 > i && j0 < R1) v0 = __builtin_fma(-a0, zi, v0);
                    if (j1 > i && j1 < R1) v1 = __builtin_fma(-a1, zi, v1);
                    a0 = n0; a1 = n1; yi = yn;
                }
                double b0 = Lm[(R1 - 1) * ld + jc0] * id0, b1 = two ? Lm[(R1 - 1) * ld + jc1] * id1 : 0.0;
                for (int i = R1 - 1; i >= 0; --i) {                // L^T p = z
                    const int in = i > 0 ? i - 1 : 0;
                    const double n0 = Lm[in * ld + jc0] * id0, n1 = two ? Lm[in * ld + jc1] * id1 : 0.0;
                    const double pi = meb_readlane(i < 64 ? v0 : v1, i & 63);
                    if (j0 < i) v0 = __builtin_fma(-b0, pi, v0);
                    if (j1 < i) v1 = __builtin_fma(-b1, pi, v1);
                    b0 = n0; b1 = n1;
                }
            }
            if (j0 < R1) pdir[j0] = v0;
            if (j1 < R1) pdir[j1] = v1;
            double gn = (j0 < R1 ? g[j0] * g[j0] : 0.0) + (j1 < R1 ? g[j1] * g[j1] : 0.0);
            double gpv = (j0 < R1 ? g[j0] * v0 : 0.0) + (j1 < R1 ? g[j1] * v1 : 0.0);
            double lpv = (j0 < R1 ? mus[j0] * v0 : 0.0) + (j1 < R1 ? mus[j1] * v1 : 0.0);
            gn = wave_sum(gn);
            gpv = wave_sum(gpv);
            lpv = wave_sum(lpv);
            if (tid == 0) {
                red[0] = sqrt(gn);
                red[1] = gpv;
                red[2] = bad_s ? 1.0 : 0.0;
                red[3] = lpv;
                red[4] = red[5];
            }
        }
        __syncthreads();
        gnorm = red[0];
        gp = red[1];
        const bool not_spd = red[2] != 0.0;
        if (!(gnorm == gnorm) || !(F == F)) break;
        if (gnorm < A.tol) { success = 1; break; }
        if (it == A.max_it || give_up) break;
        ++it;
        if (not_spd || !(gp < 0.0)) {
            tau = (tau == 0.0) ? 1e-10 * (1.0 + fabs(F)) : tau * 100.0;
            if (tau > 1e20) break;
            continue;
        }
        spec = true;
    }
    __syncthreads();
    double *o = A.out + (int64_t)pb * A.ldo;
    if (tid == 0) {
        o[0] = (double)nit;
        o[1] = (double)success;
        o[2] = F;
        o[3] = gnorm;
        o[4] = moment0;
    }
    for (int i = tid; i < R1; i += MEB_THREADS) {
        o[8 + i] = lam[i];
        o[8 + A.ldv + i] = g[i];
    }
    if (A.want_h) {
        double *H = o + 8 + 2 * (int64_t)A.ldv;
#pragma unroll
        for (int s = 0; s < MEB_NS; ++s) {
            if (tid + MEB_THREADS * s < nbp) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int l = 0; l < 4; ++l) {
                        const int r = 4 * hbi[s] + k, c = 4 * hbj[s] + l;
                        if (r < R1 && c < R1 && (hbi[s] != hbj[s] || k <= l)) {
                            H[(int64_t)r * A.ldv + c] = hacc[s][4 * k + l];
                            H[(int64_t)c * A.ldv + r] = hacc[s][4 * k + l];
                        }
                    }
            }
        }
    }
}

// the workspace shared by the batched solver and the density entries (MebWorkspace: maxent_batch.hpp)
MebWorkspace &meb_ws() {
    static MebWorkspace ws;
    return ws;
}

}  // namespace mlmc

using namespace mlmc;

extern "C" {

int mlmc_maxent_solve_batch(int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *a, const double *b,
                            const double *mu, const double *sigma, const mlmc_maxent_opts *opts, double *lambda_io,
                            double *grad_out, double *hess_out, mlmc_maxent_info *info) {
    MLMC_API_GUARD;
    static const char *fn = "mlmc_maxent_solve_batch";
    if (!rt().ready) return fail("mlmc_init has not been called (no HIP device bound)");
    if (B < 0) return fail("mlmc_maxent_solve_batch: B < 0");
    if (B == 0) return 0;
    if (!bases || !R1 || !a || !b || !mu || !sigma || !opts || !lambda_io || !info)
        return fail("mlmc_maxent_solve_batch: null argument");
    if (opts->stab_penalty != 0.0 || opts->penalty_coef != 0.0)
        return fail("mlmc_maxent_solve_batch: penalised options (stab_penalty / penalty_coef) are not supported in a batch; "
                    "use mlmc_maxent_solve");
    int ldv = 0;
    for (int i = 0; i < B; ++i) {
        const mlmc_basis *bs = bases[i];
        if (!bs) return meb_fail(fn, i, "null basis");
        if (R1[i] <= 0) return meb_fail(fn, i, "R1 = " + std::to_string(R1[i]) + " <= 0");
        if (R1[i] > MEB_MAX_R) return meb_fail(fn, i, "R1 = " + std::to_string(R1[i]) + " > 128 (at most 128 moments)");
        const int max_out = bs->out_size > 0 ? bs->out_size : bs->p.size;
        if (R1[i] > max_out) return meb_fail(fn, i, "R1 = " + std::to_string(R1[i]) + " exceeds the basis size " + std::to_string(max_out));
        if (bs->p.kind == MLMC_IDENTITY) return meb_fail(fn, i, "IDENTITY basis");
        if (bs->out_size > 0 && bs->p.size > MEB_MAX_BASE) return meb_fail(fn, i, "transformed basis over more than 512 terms");
        if (!(b[i] > a[i])) return meb_fail(fn, i, "empty domain");
        ldv = std::max(ldv, (int)R1[i]);
    }
    for (int i = 0; i < B; ++i)
        for (int j = 0; j < R1[i]; ++j)
            if (!(sigma[(size_t)i * ldv + j] > 0.0)) return meb_fail(fn, i, "sigma <= 0 (moment standard errors must be positive)");
    hipStream_t st = rt().stream;
    const int deg = opts->gauss_degree > 0 ? opts->gauss_degree : 21;
    const int nint = opts->n_intervals > 0 ? opts->n_intervals : 64;
    const int Q = deg * nint;
    const int max_it = opts->max_it > 0 ? opts->max_it : 100;
    const double tol = opts->tol > 0 ? opts->tol : 1e-8;
    const int want_h = hess_out != nullptr;
    const int QS = ldv <= 64 ? 64 : 32;
    const int T4 = (ldv + 3) / 4;
    const size_t lds_solve = sizeof(double) * ((size_t)std::max(QS * 4 * T4, ldv * (ldv + 1)) + 5 * (size_t)QS + 7 * (size_t)ldv + 16);
    if (lds_solve > (size_t)MEB_LDS_LIMIT) return fail("mlmc_maxent_solve_batch: LDS budget exceeded");
    int max_terms = 1;
    for (int i = 0; i < B; ++i) max_terms = std::max(max_terms, bases[i]->out_size > 0 ? bases[i]->p.size : (int)R1[i]);
    const size_t lds_phi = sizeof(double) * (size_t)MEB_EVAL_PTS * (max_terms + 1);

    // ---- one input block: problem table | mu / sigma | sigma | lambda | Gauss rule; one output block ----
    const size_t nv = (size_t)B * ldv;
    const int64_t ldo = 8 + 2 * (int64_t)ldv + (want_h ? (int64_t)ldv * ldv : 0);
    const size_t b_probs = meb_align(sizeof(MebProb) * B), b_vec = meb_align(sizeof(double) * nv), b_g = meb_align(sizeof(double) * deg);
    const size_t b_in = b_probs + 3 * b_vec + 2 * b_g;
    const size_t b_out = meb_align(sizeof(double) * (size_t)B * ldo);
    size_t n_phi = 0;
    std::vector<MebProb> probs(B);
    for (int i = 0; i < B; ++i) {
        const mlmc_basis *bs = bases[i];
        MebProb &p = probs[i];
        p.bp = bs->p;
        p.scale = bs->d_scale;
        p.matrix = bs->out_size > 0 ? bs->d_matrix : nullptr;
        p.n_terms = bs->out_size > 0 ? bs->p.size : R1[i];
        p.R1 = R1[i];
        p.phi_off = (int64_t)n_phi;
        p.a = a[i];
        p.b = b[i];
        n_phi += (size_t)Q * R1[i];
    }
    const size_t b_phi = meb_align(sizeof(double) * n_phi);
    MebWorkspace &ws = meb_ws();
    if (ws.reserve(b_in + b_phi + b_out, b_in + b_out)) return 1;
    char *h = ws.host, *d = ws.dev;
    std::memcpy(h, probs.data(), sizeof(MebProb) * B);
    double *h_mus = (double *)(h + b_probs), *h_sig = (double *)(h + b_probs + b_vec), *h_lam = (double *)(h + b_probs + 2 * b_vec);
    double *h_gx = (double *)(h + b_probs + 3 * b_vec), *h_gw = (double *)(h + b_probs + 3 * b_vec + b_g);
    for (int i = 0; i < B; ++i)
        for (int j = 0; j < ldv; ++j) {
            const size_t k = (size_t)i * ldv + j;
            const bool in = j < R1[i];
            h_mus[k] = in ? mu[k] / sigma[k] : 0.0;
            h_sig[k] = in ? sigma[k] : 1.0;
            h_lam[k] = in ? lambda_io[k] : 0.0;
        }
    {
        std::vector<double> gx, gw;
        gauss_legendre(deg, gx, gw);
        std::memcpy(h_gx, gx.data(), sizeof(double) * deg);
        std::memcpy(h_gw, gw.data(), sizeof(double) * deg);
    }
    const MebProb *d_probs = (const MebProb *)d;
    const double *d_mus = (const double *)(d + b_probs), *d_sig = (const double *)(d + b_probs + b_vec);
    const double *d_lam = (const double *)(d + b_probs + 2 * b_vec);
    const double *d_gx = (const double *)(d + b_probs + 3 * b_vec), *d_gw = (const double *)(d + b_probs + 3 * b_vec + b_g);
    double *d_phi = (double *)(d + b_in), *d_out = (double *)(d + b_in + b_phi);
    MLMC_HIP_CHECK(hipMemcpyAsync(d, h, b_in, hipMemcpyHostToDevice, st));
    MLMC_HIP_CHECK(hipMemsetAsync(d_out, 0, sizeof(double) * (size_t)B * ldo, st));

    MLMC_HIP_CHECK(hipFuncSetAttribute((const void *)k_meb_phi, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_phi));
    hipLaunchKernelGGL(k_meb_phi, dim3((unsigned)B, (unsigned)((Q + MEB_EVAL_PTS - 1) / MEB_EVAL_PTS)), dim3(MEB_THREADS), lds_phi, st,
                       d_probs, d_sig, ldv, d_gx, d_gw, nint, deg, d_phi);
    MLMC_HIP_CHECK(hipGetLastError());
    MebArgs A;
    A.probs = d_probs; A.phi = d_phi; A.mus = d_mus; A.sigma = d_sig; A.lam0 = d_lam; A.gx = d_gx; A.gw = d_gw;
    A.out = d_out; A.ldo = ldo; A.ldv = ldv; A.nint = nint; A.deg = deg; A.QS = QS; A.max_it = max_it; A.want_h = want_h;
    A.tol = tol;
    const int nbp_max = T4 * (T4 + 1) / 2;
    const void *kfn = nbp_max <= MEB_THREADS ? (const void *)k_meb_solve<1>
                    : nbp_max <= 2 * MEB_THREADS ? (const void *)k_meb_solve<2> : (const void *)k_meb_solve<MEB_NS_MAX>;
    MLMC_HIP_CHECK(hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_solve));
    if (nbp_max <= MEB_THREADS)
        hipLaunchKernelGGL(k_meb_solve<1>, dim3((unsigned)B), dim3(MEB_THREADS), lds_solve, st, A);
    else if (nbp_max <= 2 * MEB_THREADS)
        hipLaunchKernelGGL(k_meb_solve<2>, dim3((unsigned)B), dim3(MEB_THREADS), lds_solve, st, A);
    else
        hipLaunchKernelGGL(k_meb_solve<MEB_NS_MAX>, dim3((unsigned)B), dim3(MEB_THREADS), lds_solve, st, A);
    MLMC_HIP_CHECK(hipGetLastError());
    double *res = (double *)(h + b_in);
    MLMC_HIP_CHECK(hipMemcpyAsync(res, d_out, sizeof(double) * (size_t)B * ldo, hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(wait_stream(st));

    for (int i = 0; i < B; ++i) {
        const double *o = res + (size_t)i * ldo;
        std::memcpy(lambda_io + (size_t)i * ldv, o + 8, sizeof(double) * R1[i]);
        if (grad_out) std::memcpy(grad_out + (size_t)i * ldv, o + 8 + ldv, sizeof(double) * ldv);
        if (hess_out) std::memcpy(hess_out + (size_t)i * ldv * ldv, o + 8 + 2 * (size_t)ldv, sizeof(double) * (size_t)ldv * ldv);
        info[i].nit = (int)o[0];
        info[i].success = (int)o[1];
        info[i].fun = o[2];
        info[i].grad_norm = o[3];
        info[i].moment0 = o[4];
        info[i].n_quad = Q;
        info[i].reserved = 0;
    }
    ws.trim(MEB_KEEP_BYTES);
    return 0;
}

}  // extern "C"
