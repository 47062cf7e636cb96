// Per-level MLMC convergence diagnostics of every component of a vector quantity (gfx950): central sums up to order 4 of the
// level differences, mean and second central sum of the fine and of the coarse values, and their co-moment.
//
// Per (level l, component m) and kept sample (neither the fine nor -- with a coarse row -- the coarse value is NaN):
//     y = fl(f - c)  (no coarse row: y = f),   M_k(x) = sum (x - mean(x))^k,   C_fc = sum (f - mean f)(c - mean c)
//     stats = mean_y, M2_y, M3_y, M4_y, mean_f, M2_f, mean_c, M2_c, C_fc        (MLMC_DIAG_NSTAT = 9)
// Two passes over a chunk, so that no sum cancels: k_diag_sums gives sum y, sum f, sum c and the counts, k_diag_pivot the
// pivots p = sum / n; k_diag_central sums the powers of d = x - p (|mean d| is at rounding level of the data, so the sums are
// those of the central moments up to a correction of relative size (mean d / sd)), and k_diag_finish applies that correction
// exactly (binomial expansion about mean d = S1 / n).  A chunk that fits the last-level cache is read from HBM once; a larger
// one (a level of 64 x 10^6 pairs is 1 GB) streams from HBM in both passes.
// Grid (sample block, component); a lane takes two neighbouring samples per trip (one 16-byte load per row) and keeps its sums in
// registers in index order; wave butterfly, the four waves in order, then one workgroup per component adds the block partials
// in a fixed strided order.  The samples per block depend on n alone: a component's bits do not depend on M or on its row.
// The chunks of a level are merged on the host, in the order of the call, by the pairwise updates of Chan et al. / Pebay
// (mlmc_diag_merge).
#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "device_basis.hpp"

namespace mlmc {

constexpr int LD_THREADS = 256;
constexpr int LD_TRIP = 2 * LD_THREADS;       // samples of one trip of a workgroup
constexpr int LD_MAX_BLOCKS = 1024;           // sample blocks per component and chunk
constexpr int64_t LD_MIN_PER = 2048;          // samples per block at least
constexpr int LD_NSUM = 3;                    // first pass: sum y, sum f, sum c
constexpr int LD_NCEN = 9;                    // second pass: S1..S4 of y, S1, S2 of f, S1, S2 of c, sum df dc
constexpr int LD_MAX_M = 65535;               // grid.y
constexpr size_t LD_SCRATCH = size_t(64) << 20;

// samples per block of a chunk of n samples (a multiple of LD_TRIP: every block but the last starts on a lane-pair boundary)
static int64_t ld_per(int64_t n) {
    int64_t per = (n + LD_MAX_BLOCKS - 1) / LD_MAX_BLOCKS;
    per = (per + LD_TRIP - 1) / LD_TRIP * LD_TRIP;
    return std::max(per, LD_MIN_PER);
}
static int ld_blocks(int64_t n) { return (int)((n + ld_per(n) - 1) / ld_per(n)); }

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <bool AL>
__device__ __forceinline__ double2 ld_load2(const double *__restrict__ p) {
    if (AL) return *reinterpret_cast<const double2 *>(p);
    return make_double2(p[0], p[1]);
}

// use(f, c) for the samples [s0, s1) of this workgroup: lane t takes s0 + 2 t, s0 + 2 t + 1 of every trip, in index order
// whatever the alignment of the rows (AL: both rows 16-byte aligned at s0, one load per pair).  Two trips are in flight.
template <bool PAIR, bool AL, class Use>
__device__ __forceinline__ void ld_for_each(const double *__restrict__ f, const double *__restrict__ c, int64_t s0, int64_t s1,
                                            Use &&use) {
    int64_t i = s0 + 2 * (int64_t)threadIdx.x;
    const int64_t full = s0 + (s1 - s0) / (2 * LD_TRIP) * (2 * LD_TRIP);     // end of the whole double trips
    for (; i < full; i += 2 * LD_TRIP) {
        const double2 fa = ld_load2<AL>(f + i), fb = ld_load2<AL>(f + i + LD_TRIP);
        double2 ca = make_double2(0.0, 0.0), cb = ca;
        if (PAIR) { ca = ld_load2<AL>(c + i); cb = ld_load2<AL>(c + i + LD_TRIP); }
        use(fa.x, ca.x);
        use(fa.y, ca.y);
        use(fb.x, cb.x);
        use(fb.y, cb.y);
    }
    for (; i < s1; i += LD_TRIP) {                                           // the last (at most two) trips, bounds checked
        if (i + 1 < s1) {
            const double2 fa = ld_load2<AL>(f + i);
            const double2 ca = PAIR ? ld_load2<AL>(c + i) : make_double2(0.0, 0.0);
            use(fa.x, ca.x);
            use(fa.y, ca.y);
        } else {
            use(f[i], PAIR ? c[i] : 0.0);
        }
    }
}

template <bool PAIR>
__device__ __forceinline__ bool ld_aligned(const double *f, const double *c, int64_t s0) {
    return ((reinterpret_cast<uintptr_t>(f + s0) | (PAIR ? reinterpret_cast<uintptr_t>(c + s0) : 0)) & 15) == 0;
}

// tot[j] (every thread) = v[j] summed over the workgroup: wave butterfly, then the four waves in order
template <int NS>
__device__ __forceinline__ void ld_workgroup_sums(const double (&v)[NS], double (&red)[4][NS], double (&tot)[NS]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const double w = wave_sum(v[j]);
        if (lane == 0) red[wave][j] = w;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NS; ++j) tot[j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
}

// ... written to out[0..NS) by thread 0: a block partial
template <int NS>
__device__ __forceinline__ void ld_block_sums(const double (&v)[NS], double (&red)[4][NS], double *__restrict__ out) {
    double tot[NS];
    ld_workgroup_sums<NS>(v, red, tot);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NS; ++j) out[j] = tot[j];
    }
}

// first pass.  part[(m * nb + b) * 3 + {0, 1, 2}] = block b's sum y, sum f, sum c of component m over its kept samples;
// pcount[(m * nb + b) * 2 + {0, 1}] = kept / dropped
template <bool PAIR>
__global__ __launch_bounds__(LD_THREADS) void k_diag_sums(const double *__restrict__ fine, const double *__restrict__ coarse, int64_t n,
                                                          int64_t per, int nb, double *__restrict__ part, int64_t *__restrict__ pcount) {
    const int b = blockIdx.x, m = blockIdx.y;
    const int64_t s0 = std::min<int64_t>(n, (int64_t)b * per), s1 = std::min<int64_t>(n, s0 + per);
    const double *f = fine + (int64_t)m * n;
    const double *c = PAIR ? coarse + (int64_t)m * n : nullptr;
    double v[LD_NSUM] = {0.0, 0.0, 0.0};
    int kept = 0;
    auto use = [&](double xf, double xc) {
        const bool keep = xf == xf && (!PAIR || xc == xc);
        kept += keep;
        v[0] += keep ? xf - xc : 0.0;
        if (PAIR) {
            v[1] += keep ? xf : 0.0;
            v[2] += keep ? xc : 0.0;
        }
    };
    if (ld_aligned<PAIR>(f, c, s0)) ld_for_each<PAIR, true>(f, c, s0, s1, use);
    else ld_for_each<PAIR, false>(f, c, s0, s1, use);
    __shared__ double red[4][LD_NSUM];
    __shared__ int cred[4];
    kept = wave_sum_i(kept);
    if ((threadIdx.x & 63) == 0) cred[threadIdx.x >> 6] = kept;
    ld_block_sums<LD_NSUM>(v, red, part + ((int64_t)m * nb + b) * LD_NSUM);
    if (threadIdx.x == 0) {
        const int64_t k = ((int64_t)cred[0] + cred[1]) + ((int64_t)cred[2] + cred[3]);
        pcount[((int64_t)m * nb + b) * 2] = k;
        pcount[((int64_t)m * nb + b) * 2 + 1] = (s1 - s0) - k;
    }
}

// tot[j] (every thread) = sum over the blocks of part[(m * nb + b) * NS + j]: thread t adds the blocks t, t + 256, ... in order,
// then the workgroup sum
template <int NS>
__device__ __forceinline__ void ld_merge_blocks(const double *__restrict__ part, int m, int nb, double (&red)[4][NS], double (&tot)[NS]) {
    double v[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) v[j] = 0.0;
    for (int b = threadIdx.x; b < nb; b += LD_THREADS) {
#pragma unroll
        for (int j = 0; j < NS; ++j) v[j] += part[((int64_t)m * nb + b) * NS + j];
    }
    ld_workgroup_sums<NS>(v, red, tot);
}

// pivots[m * 3 + j] = (sum y, sum f, sum c) / kept (0 without a kept sample); counts[m * 2 + {0, 1}] = kept / dropped of the chunk
__global__ __launch_bounds__(LD_THREADS) void k_diag_pivot(const double *__restrict__ part, const int64_t *__restrict__ pcount, int nb,
                                                           double *__restrict__ pivots, int64_t *__restrict__ counts) {
    const int m = blockIdx.x;
    __shared__ double red[4][LD_NSUM];
    __shared__ long long cred[4][2];
    double tot[LD_NSUM];
    ld_merge_blocks<LD_NSUM>(part, m, nb, red, tot);
    long long k = 0, r = 0;
    for (int b = threadIdx.x; b < nb; b += LD_THREADS) {
        k += pcount[((int64_t)m * nb + b) * 2];
        r += pcount[((int64_t)m * nb + b) * 2 + 1];
    }
    k = wave_sum_ll(k);
    r = wave_sum_ll(r);
    if ((threadIdx.x & 63) == 0) { cred[threadIdx.x >> 6][0] = k; cred[threadIdx.x >> 6][1] = r; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long kept = cred[0][0] + cred[1][0] + cred[2][0] + cred[3][0];
        counts[(int64_t)m * 2] = kept;
        counts[(int64_t)m * 2 + 1] = cred[0][1] + cred[1][1] + cred[2][1] + cred[3][1];
#pragma unroll
        for (int j = 0; j < LD_NSUM; ++j) pivots[(int64_t)m * LD_NSUM + j] = kept > 0 ? tot[j] / (double)kept : 0.0;
    }
}

// second pass.  part[(m * nb + b) * NS + j], d = x - pivot over the kept samples: j = 0..3: sum dy^(j+1); PAIR (NS = 9): 4, 5: sum df,
// df^2; 6, 7: sum dc, dc^2; 8: sum df dc
template <bool PAIR>
__global__ __launch_bounds__(LD_THREADS) void k_diag_central(const double *__restrict__ fine, const double *__restrict__ coarse, int64_t n,
                                                             int64_t per, int nb, const double *__restrict__ pivots,
                                                             double *__restrict__ part) {
    constexpr int NS = PAIR ? LD_NCEN : 4;
    const int b = blockIdx.x, m = blockIdx.y;
    const int64_t s0 = std::min<int64_t>(n, (int64_t)b * per), s1 = std::min<int64_t>(n, s0 + per);
    const double *f = fine + (int64_t)m * n;
    const double *c = PAIR ? coarse + (int64_t)m * n : nullptr;
    const double py = pivots[(int64_t)m * LD_NSUM], pf = pivots[(int64_t)m * LD_NSUM + 1], pc = pivots[(int64_t)m * LD_NSUM + 2];
    double v[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) v[j] = 0.0;
    auto use = [&](double xf, double xc) {
        const bool keep = xf == xf && (!PAIR || xc == xc);
        const double dy = keep ? (xf - xc) - py : 0.0;          // a dropped sample yields exactly 0 in every sum
        const double dy2 = dy * dy;
        v[0] += dy;
        v[1] = __builtin_fma(dy, dy, v[1]);
        v[2] = __builtin_fma(dy2, dy, v[2]);
        v[3] = __builtin_fma(dy2, dy2, v[3]);
        if (PAIR) {
            const double df = keep ? xf - pf : 0.0, dc = keep ? xc - pc : 0.0;
            v[4] += df;
            v[5] = __builtin_fma(df, df, v[5]);
            v[6] += dc;
            v[7] = __builtin_fma(dc, dc, v[7]);
            v[8] = __builtin_fma(df, dc, v[8]);
        }
    };
    if (ld_aligned<PAIR>(f, c, s0)) ld_for_each<PAIR, true>(f, c, s0, s1, use);
    else ld_for_each<PAIR, false>(f, c, s0, s1, use);
    __shared__ double red[4][NS];
    ld_block_sums<NS>(v, red, part + ((int64_t)m * nb + b) * NS);
}

__device__ __forceinline__ double ld_mean(double p, double e) { return p - p == 0.0 ? p + e : p; }     // p - p == 0: p is finite

// central sums about the mean from the sums S_k of d^k about a pivot p, n samples: with e = S1 / n the mean is p + e and
// sum (d - e)^k expands binomially (sum of the e^k terms folded: n e = S1).  Rounding may leave M2, M4 of constant data just
// below zero: clamped (a NaN stays).  A kept +-inf makes the pivot +-inf (NaN with both signs) and every d NaN: the mean is then
// the pivot itself, sum / n, as estimate_mean gives it, and the central sums are NaN.
__device__ __forceinline__ void ld_about_mean(double n, double p, double S1, double S2, double S3, double S4, double &mean, double &M2,
                                              double &M3, double &M4) {
    const double e = S1 / n;
    mean = ld_mean(p, e);
    M2 = S2 - S1 * e;
    M3 = (S3 - 3.0 * e * S2) + 2.0 * e * e * S1;
    M4 = ((S4 - 4.0 * e * S3) + 6.0 * e * e * S2) - 3.0 * e * e * e * S1;
    M2 = M2 < 0.0 ? 0.0 : M2;
    M4 = M4 < 0.0 ? 0.0 : M4;
}

// stats[m * 9 + s] of the chunk (MLMC_DIAG_NSTAT values in the order of mlmc_hip.h); without a coarse row the fine statistics
// are those of y and the last three are NaN; without a kept sample all nine are NaN
template <bool PAIR>
__global__ __launch_bounds__(LD_THREADS) void k_diag_finish(const double *__restrict__ part, int nb, const double *__restrict__ pivots,
                                                            const int64_t *__restrict__ counts, double *__restrict__ stats) {
    constexpr int NS = PAIR ? LD_NCEN : 4;
    const int m = blockIdx.x;
    __shared__ double red[4][NS];
    double S[NS];
    ld_merge_blocks<NS>(part, m, nb, red, S);
    if (threadIdx.x != 0) return;
    double *out = stats + (int64_t)m * MLMC_DIAG_NSTAT;
    const double nan = __builtin_nan("");
    const int64_t kept = counts[(int64_t)m * 2];
    if (kept == 0) {
#pragma unroll
        for (int s = 0; s < MLMC_DIAG_NSTAT; ++s) out[s] = nan;
        return;
    }
    const double n = (double)kept;
    ld_about_mean(n, pivots[(int64_t)m * LD_NSUM], S[0], S[1], S[2], S[3], out[0], out[1], out[2], out[3]);
    if (PAIR) {
        const double ef = S[4] / n, ec = S[6] / n;
        double M2f = S[5] - S[4] * ef, M2c = S[7] - S[6] * ec;
        out[4] = ld_mean(pivots[(int64_t)m * LD_NSUM + 1], ef);
        out[5] = M2f < 0.0 ? 0.0 : M2f;
        out[6] = ld_mean(pivots[(int64_t)m * LD_NSUM + 2], ec);
        out[7] = M2c < 0.0 ? 0.0 : M2c;
        out[8] = S[8] - S[4] * ec;
    } else {
        out[4] = out[0];
        out[5] = out[1];
        out[6] = out[7] = out[8] = nan;
    }
}

// The nine statistics of the union of two disjoint sample sets (a: na samples, b: nb): Chan, Golub, LeVeque (1983) for the mean
// and M2, Pebay (2008) for M3, M4 and the co-moment, evaluated in the host's long double.
static void diag_merge(const double *a, int64_t na, const double *b, int64_t nb, double *out) {
    if (na <= 0 || nb <= 0) {
        const double *src = nb <= 0 ? a : b;
        double tmp[MLMC_DIAG_NSTAT];
        for (int s = 0; s < MLMC_DIAG_NSTAT; ++s) tmp[s] = src[s];
        for (int s = 0; s < MLMC_DIAG_NSTAT; ++s) out[s] = tmp[s];
        return;
    }
    typedef long double ld;
    const ld A = (ld)na, B = (ld)nb, N = A + B;
    const ld d = (ld)b[0] - (ld)a[0], d2 = d * d;
    const ld M2a = a[1], M2b = b[1], M3a = a[2], M3b = b[2], M4a = a[3], M4b = b[3];
    // the mean of the union; a side with a kept +-inf has that mean (the update by the difference would give inf - inf)
    auto mean = [&](ld ma, ld mb, ld diff) { return diff - diff == 0.0L ? ma + diff * B / N : (A * ma + B * mb) / N; };
    double r[MLMC_DIAG_NSTAT];
    r[0] = (double)mean(a[0], b[0], d);
    r[1] = (double)(M2a + M2b + d2 * A * B / N);
    r[2] = (double)(M3a + M3b + d2 * d * A * B * (A - B) / (N * N) + 3.0L * d * (A * M2b - B * M2a) / N);
    r[3] = (double)(M4a + M4b + d2 * d2 * A * B * (A * A - A * B + B * B) / (N * N * N) +
                    6.0L * d2 * (A * A * M2b + B * B * M2a) / (N * N) + 4.0L * d * (A * M3b - B * M3a) / N);
    const ld df = (ld)b[4] - (ld)a[4], dc = (ld)b[6] - (ld)a[6];
    r[4] = (double)mean(a[4], b[4], df);
    r[5] = (double)((ld)a[5] + (ld)b[5] + df * df * A * B / N);
    r[6] = (double)mean(a[6], b[6], dc);
    r[7] = (double)((ld)a[7] + (ld)b[7] + dc * dc * A * B / N);
    r[8] = (double)((ld)a[8] + (ld)b[8] + df * dc * A * B / N);
    for (int s = 0; s < MLMC_DIAG_NSTAT; ++s) out[s] = r[s];
}

}  // namespace mlmc

using namespace mlmc;

extern "C" {

int mlmc_diag_merge(const double *a, int64_t na, const double *b, int64_t nb, double *out) {
    if (!a || !b || !out) return fail("mlmc_diag_merge: null argument");
    if (na < 0 || nb < 0) return fail("mlmc_diag_merge: negative sample count");
    diag_merge(a, na, b, nb, out);
    return 0;
}

int mlmc_level_diagnostics(int32_t M, int32_t n_levels, int32_t n_chunks, const int32_t *levels, const double *const *fine,
                           const double *const *coarse, const int64_t *n_samples, int64_t *n_out, int64_t *n_rm_out,
                           double *stats_out) {
    MLMC_API_GUARD;
    const std::string e("mlmc_level_diagnostics");
    if (!rt().ready) return fail("mlmc_init has not been called (no HIP device bound)");
    if (M < 1 || M > LD_MAX_M || n_levels <= 0 || n_chunks < 0) return fail(e + ": bad M / n_levels / n_chunks");
    if (!n_out || !n_rm_out || !stats_out || (n_chunks > 0 && (!levels || !fine || !coarse || !n_samples)))
        return fail(e + ": null argument");
    // a level is of one kind: pairs, or fine values alone (level 0 always: its coarse pointers are not read)
    std::vector<signed char> kind(n_levels, -1);
    std::vector<char> pair(std::max(n_chunks, 1), 0);
    int64_t n_max = 0;
    for (int c = 0; c < n_chunks; ++c) {
        if (levels[c] < 0 || levels[c] >= n_levels) return fail(e + ": chunk level out of range");
        if (n_samples[c] < 0 || (n_samples[c] > 0 && !fine[c])) return fail(e + ": bad chunk");
        pair[c] = levels[c] > 0 && coarse[c] != nullptr;
        if (n_samples[c] == 0) continue;
        signed char &k = kind[levels[c]];
        if (k >= 0 && k != pair[c])
            return fail(e + ": level " + std::to_string(levels[c]) + " has chunks with and without coarse samples");
        k = pair[c];
        n_max = std::max(n_max, n_samples[c]);
    }
    const int64_t L = n_levels;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int64_t i = 0; i < L * M; ++i) n_out[i] = n_rm_out[i] = 0;
    for (int64_t i = 0; i < L * M * MLMC_DIAG_NSTAT; ++i) stats_out[i] = nan;
    if (n_max == 0) return 0;

    hipStream_t st = rt().stream;
    // scratch of a group of mg components (block partials of both passes, pivots) within LD_SCRATCH, and the per-chunk results
    const int nb_max = ld_blocks(n_max);
    const size_t per_comp = (size_t)nb_max * (LD_NSUM + LD_NCEN + 2) * 8;
    const int64_t Mg = std::max<int64_t>(1, std::min<int64_t>(M, (int64_t)(LD_SCRATCH / per_comp)));
    const size_t b_p1 = mm_align(sizeof(double) * (size_t)Mg * nb_max * LD_NSUM), b_pc = mm_align(sizeof(int64_t) * (size_t)Mg * nb_max * 2);
    const size_t b_p2 = mm_align(sizeof(double) * (size_t)Mg * nb_max * LD_NCEN), b_piv = mm_align(sizeof(double) * (size_t)Mg * LD_NSUM);
    const size_t b_st = mm_align(sizeof(double) * (size_t)n_chunks * M * MLMC_DIAG_NSTAT);
    const size_t b_ct = mm_align(sizeof(int64_t) * (size_t)n_chunks * M * 2);
    static MultiWorkspace ws;
    if (ws.reserve(b_p1 + b_pc + b_p2 + b_piv + b_st + b_ct)) return 1;
    char *p = ws.dev;
    double *d_p1 = (double *)p;
    int64_t *d_pc = (int64_t *)(p += b_p1);
    double *d_p2 = (double *)(p += b_pc);
    double *d_piv = (double *)(p += b_p2);
    double *d_stats = (double *)(p += b_piv);
    int64_t *d_counts = (int64_t *)(p += b_st);
    for (int c = 0; c < n_chunks; ++c) {
        const int64_t n = n_samples[c];
        if (n == 0) continue;
        const int64_t per = ld_per(n);
        const int nb = ld_blocks(n);
        for (int64_t g0 = 0; g0 < M; g0 += Mg) {
            const int64_t mg = std::min<int64_t>(Mg, M - g0);
            const double *f = fine[c] + g0 * n;
            const double *co = pair[c] ? coarse[c] + g0 * n : nullptr;
            double *d_s = d_stats + ((size_t)c * M + g0) * MLMC_DIAG_NSTAT;
            int64_t *d_c = d_counts + ((size_t)c * M + g0) * 2;
            const dim3 grid((unsigned)nb, (unsigned)mg), thr(LD_THREADS);
            if (pair[c]) {
                hipLaunchKernelGGL(k_diag_sums<true>, grid, thr, 0, st, f, co, n, per, nb, d_p1, d_pc);
                hipLaunchKernelGGL(k_diag_pivot, dim3((unsigned)mg), thr, 0, st, d_p1, d_pc, nb, d_piv, d_c);
                hipLaunchKernelGGL(k_diag_central<true>, grid, thr, 0, st, f, co, n, per, nb, d_piv, d_p2);
                hipLaunchKernelGGL(k_diag_finish<true>, dim3((unsigned)mg), thr, 0, st, d_p2, nb, d_piv, d_c, d_s);
            } else {
                hipLaunchKernelGGL(k_diag_sums<false>, grid, thr, 0, st, f, co, n, per, nb, d_p1, d_pc);
                hipLaunchKernelGGL(k_diag_pivot, dim3((unsigned)mg), thr, 0, st, d_p1, d_pc, nb, d_piv, d_c);
                hipLaunchKernelGGL(k_diag_central<false>, grid, thr, 0, st, f, co, n, per, nb, d_piv, d_p2);
                hipLaunchKernelGGL(k_diag_finish<false>, dim3((unsigned)mg), thr, 0, st, d_p2, nb, d_piv, d_c, d_s);
            }
            MLMC_HIP_CHECK(hipGetLastError());
        }
    }
    // (chunks without samples were not launched: their rows of h_stats / h_counts are never read)
    std::vector<double> h_stats((size_t)n_chunks * M * MLMC_DIAG_NSTAT);
    std::vector<int64_t> h_counts((size_t)n_chunks * M * 2);
    MLMC_HIP_CHECK(hipMemcpyAsync(h_stats.data(), d_stats, sizeof(double) * h_stats.size(), hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(hipMemcpyAsync(h_counts.data(), d_counts, sizeof(int64_t) * h_counts.size(), hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(wait_stream(st));
    for (int c = 0; c < n_chunks; ++c) {
        if (n_samples[c] == 0) continue;
        for (int64_t m = 0; m < M; ++m) {
            const size_t lm = (size_t)(levels[c] * (int64_t)M + m), cm = (size_t)c * M + m;
            double *acc = stats_out + lm * MLMC_DIAG_NSTAT;
            diag_merge(acc, n_out[lm], h_stats.data() + cm * MLMC_DIAG_NSTAT, h_counts[cm * 2], acc);
            n_out[lm] += h_counts[cm * 2];
            n_rm_out[lm] += h_counts[cm * 2 + 1];
        }
    }
    return 0;
}

}  // extern "C"
