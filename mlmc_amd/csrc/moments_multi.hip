// Per-component moment sums of a vector quantity (gfx950): M basis descriptors, ONE pass over each stored chunk, with or
// without the sums of squares (SQ: the level variances).
//
// Estimate.construct_densities needs, per scalar component m, the level sums of K = linearize.extended_size(fn_m) moments of
// fn_m's family (the covariance mean by the product linearisation, the orthogonal-moments mean as T_m times the first R of
// them) -- each component masked and clipped ON ITS OWN; the per-component moment estimates need the sums of squares too.  The
// scalar chain runs its estimates per component; here one launch per (level, chunk) -- two with K > 32 -- covers every
// component: grid (sample block, component, 32-term window), the component's BasisParams from a device table, the window's
// sums in registers, fixed-order wave / block reductions, and a fixed-order merge of the block partials into the level totals
// (k_multi_reduce), so the sums are the same bits run to run, and Σd is the same bits with and without Σd².
// Keep rule per component = the scalar path's for a one-component chunk: transform_value keeps the fine value AND (above
// level 0) the coarse value; a NaN is never kept.  The counts are therefore bit-identical to the scalar chain's.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "device_basis.hpp"

namespace mlmc {

constexpr int MM_THREADS = 256;
constexpr int MM_MAX_K = 512;
constexpr int MV_WIN = 32;            // terms per window with K > 16 (Σd and Σd²: 128 VGPRs)

// Σd (and with SQ Σd²) of up to NW terms of one component per workgroup, grid (sample block, component, term window).  Each
// lane takes two samples per trip (four independent recurrences for a fine / coarse pair) and issues the next trip's loads
// before the current trip's arithmetic, as the scalar kernel does (moments.hip, accum_samples).  The tile is computed whole:
// terms >= K of the last window are evaluated and discarded (no run-time guard inside the unrolled loop).  A window at k0 > 0
// first walks the k0 terms before it -- the first 32 with compile-time coefficients, the rest in blocks of 32 whose Legendre
// coefficients are fetched ahead of the dependent steps -- and accumulates its own terms the same way.
template <bool SQ>
__device__ __forceinline__ void mv_add(double d, double &s, double &sp) {
    s += d;
    if constexpr (SQ) sp = __builtin_fma(d, d, sp);
}

template <int KIND, int NW, bool PAIR, bool FIRST, bool SQ>
__device__ __forceinline__ void mv_accumulate(const BasisParams &bp, const double *__restrict__ f, const double *__restrict__ c,
                                              int64_t s0, int64_t s1, int k0, double (&s)[NW], double (&sp)[SQ ? NW : 1],
                                              int &kept, int &removed) {
    constexpr int64_t T = MM_THREADS;
    int64_t i0 = s0 + threadIdx.x, i1 = i0 + T;
    double f0 = 0.0, f1 = 0.0, c0 = 0.0, c1 = 0.0;
    if (i0 < s1) { f0 = f[i0]; if (PAIR) c0 = c[i0]; }
    if (i1 < s1) { f1 = f[i1]; if (PAIR) c1 = c[i1]; }
    while (i0 < s1) {
        const bool v1 = i1 < s1;
        const double xf0 = f0, xf1 = f1, xc0 = c0, xc1 = c1;
        // prefetch the next trip: unconditional loads on a clamped index (a load under a lane mask waits where it is issued)
        const int64_t j0 = i0 + 2 * T, j1 = i1 + 2 * T, l0 = std::min(j0, s1 - 1), l1 = std::min(j1, s1 - 1);
        f0 = f[l0];
        f1 = f[l1];
        if (PAIR) { c0 = c[l0]; c1 = c[l1]; }

        bool kf0, kf1, kc0 = true, kc1 = true;
        const double tf0 = transform_value(bp, xf0, kf0);
        const double tf1 = transform_value(bp, xf1, kf1);
        double tc0 = 0.0, tc1 = 0.0;
        if (PAIR) {
            tc0 = transform_value(bp, xc0, kc0);
            tc1 = transform_value(bp, xc1, kc1);
        }
        const bool k0s = kf0 && kc0, k1s = v1 && kf1 && kc1;
        kept += (int)k0s + (int)k1s;
        removed += (int)(!k0s) + (int)(v1 && !k1s);
        const double w0 = k0s ? 1.0 : 0.0, w1 = k1s ? 1.0 : 0.0;   // a dropped sample yields exactly 0 in every term
        TermGen<KIND> gf0, gf1, gc0, gc1;
        gf0.init(k0s ? tf0 : 0.0, w0, bp);
        gf1.init(k1s ? tf1 : 0.0, w1, bp);
        if (PAIR) { gc0.init(k0s ? tc0 : 0.0, w0, bp); gc1.init(k1s ? tc1 : 0.0, w1, bp); }

        if constexpr (FIRST) {
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                double d0 = gf0.next(i), d1 = gf1.next(i);
                if (PAIR) { d0 -= gc0.next(i); d1 -= gc1.next(i); }
                mv_add<SQ>(d0, s[i], sp[SQ ? i : 0]);
                mv_add<SQ>(d1, s[i], sp[SQ ? i : 0]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < MV_WIN; ++i) {              // terms [0, 32) without accumulating
                gf0.next(i); gf1.next(i);
                if (PAIR) { gc0.next(i); gc1.next(i); }
            }
            for (int b = MV_WIN; b < k0; b += MV_WIN) {     // terms [32, k0)
                double gb[MV_WIN];
#pragma unroll
                for (int j = 0; j < MV_WIN; ++j) gb[j] = KIND == MLMC_LEGENDRE ? kLegendreG.v[b + j] : 0.0;
#pragma unroll
                for (int j = 0; j < MV_WIN; ++j) {
                    gf0.skip(j, gb[j]); gf1.skip(j, gb[j]);
                    if (PAIR) { gc0.skip(j, gb[j]); gc1.skip(j, gb[j]); }
                }
            }
            double ga[NW];
#pragma unroll
            for (int j = 0; j < NW; ++j) ga[j] = KIND == MLMC_LEGENDRE ? kLegendreG.v[k0 + j] : 0.0;
#pragma unroll
            for (int i = 0; i < NW; ++i) {                  // the window's terms [k0, k0 + NW), k0 a multiple of 32
                double d0 = gf0.skip(i, ga[i]), d1 = gf1.skip(i, ga[i]);
                if (PAIR) { d0 -= gc0.skip(i, ga[i]); d1 -= gc1.skip(i, ga[i]); }
                mv_add<SQ>(d0, s[i], sp[SQ ? i : 0]);
                mv_add<SQ>(d1, s[i], sp[SQ ? i : 0]);
            }
        }
        i0 = j0;
        i1 = j1;
    }
}

// part / part_sq[(m * nb + b) * K + k] = block b's Σd / Σd² of term k of component m (part_sq with SQ only);
// pcount[(m * nb + b) * 2 + {0, 1}] = kept / dropped.  Component m of the chunk is row m of fine / coarse ([M][n], n samples
// per row).
template <int KIND, int NW, bool PAIR, bool FIRST, bool SQ>
__global__ __launch_bounds__(MM_THREADS) void k_moments_multi_var(const BasisParams *__restrict__ bps, const double *__restrict__ fine,
                                                                  const double *__restrict__ coarse, int64_t n, int K, int nb,
                                                                  double *__restrict__ part, double *__restrict__ part_sq,
                                                                  int64_t *__restrict__ pcount) {
    constexpr int NC = SQ ? 2 * NW : NW;        // columns of the block reduction
    const int b = blockIdx.x, m = blockIdx.y, k0 = (blockIdx.z + (FIRST ? 0 : 1)) * MV_WIN;
    const BasisParams bp = bps[m];
    const int64_t per = (n + nb - 1) / nb, s0 = std::min<int64_t>(n, (int64_t)b * per), s1 = std::min<int64_t>(n, s0 + per);
    const double *f = fine + (int64_t)m * n;
    const double *c = PAIR ? coarse + (int64_t)m * n : nullptr;
    double s[NW], sp[SQ ? NW : 1];
#pragma unroll
    for (int j = 0; j < NW; ++j) s[j] = sp[SQ ? j : 0] = 0.0;
    int kept = 0, removed = 0;
    mv_accumulate<KIND, NW, PAIR, FIRST, SQ>(bp, f, c, s0, s1, k0, s, sp, kept, removed);
    // block partial: wave sums (fixed butterfly), then the four waves in order
    __shared__ double red[4][NC];
    __shared__ int cred[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        double v = wave_sum(s[j]), vq = 0.0;
        if constexpr (SQ) vq = wave_sum(sp[j]);
        if (lane == 0) {
            red[wave][j] = v;
            if constexpr (SQ) red[wave][NW + j] = vq;
        }
    }
    kept = wave_sum_i(kept);
    removed = wave_sum_i(removed);
    if (lane == 0) { cred[wave][0] = kept; cred[wave][1] = removed; }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < NC) {
        const int j = t < NW ? t : t - NW;
        if (k0 + j < K) {
            const double v = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
            (!SQ || t < NW ? part : part_sq)[((int64_t)m * nb + b) * K + k0 + j] = v;
        }
    }
    if (FIRST && t < 2)
        pcount[((int64_t)m * nb + b) * 2 + t] = ((int64_t)cred[0][t] + cred[1][t]) + ((int64_t)cred[2][t] + cred[3][t]);
}

// tot / tot_sq[m * K + k] += Σ_b part / part_sq[(m * nb + b) * K + k] in block order (one workgroup per component; the
// squares with SQ only, as values K .. 2K - 1 of the thread loop), counts likewise
template <bool SQ>
__global__ __launch_bounds__(MM_THREADS) void k_multi_reduce(const double *__restrict__ part, const double *__restrict__ part_sq,
                                                             const int64_t *__restrict__ pcount, int K, int nb,
                                                             double *__restrict__ tot, double *__restrict__ tot_sq,
                                                             int64_t *__restrict__ tcount) {
    const int m = blockIdx.x;
    for (int k = threadIdx.x; k < (SQ ? 2 : 1) * K; k += MM_THREADS) {
        const bool sq = SQ && k >= K;
        const double *src = sq ? part_sq : part;
        const int kk = sq ? k - K : k;
        double s = 0.0;
        for (int b = 0; b < nb; ++b) s += src[((int64_t)m * nb + b) * K + kk];
        (sq ? tot_sq : tot)[(int64_t)m * K + kk] += s;
    }
    if (threadIdx.x < 2) {
        int64_t s = 0;
        for (int b = 0; b < nb; ++b) s += pcount[((int64_t)m * nb + b) * 2 + threadIdx.x];
        tcount[(int64_t)m * 2 + threadIdx.x] += s;
    }
}

// (kind, tile, pair, sq) -> the instantiation of k_moments_multi_var; tile 0: the 16-term tile of K <= 16, 1: the first
// 32-term window, 2: the windows after the first (FIRST = false)
using MultiFn = void (*)(const BasisParams *, const double *, const double *, int64_t, int, int, double *, double *, int64_t *);

static MultiFn multi_kernel(int kind, int tile, bool pair, bool sq) {
#define MV_CELL(KIND, NW, FIRST)                                                                                         \
    {{k_moments_multi_var<KIND, NW, false, FIRST, false>, k_moments_multi_var<KIND, NW, false, FIRST, true>},            \
     {k_moments_multi_var<KIND, NW, true, FIRST, false>, k_moments_multi_var<KIND, NW, true, FIRST, true>}}
#define MV_KIND(KIND) {MV_CELL(KIND, 16, true), MV_CELL(KIND, MV_WIN, true), MV_CELL(KIND, MV_WIN, false)}
    static const MultiFn fn[3][3][2][2] = {MV_KIND(MLMC_LEGENDRE), MV_KIND(MLMC_MONOMIAL), MV_KIND(MLMC_FOURIER)};
#undef MV_KIND
#undef MV_CELL
    return fn[kind == MLMC_LEGENDRE ? 0 : (kind == MLMC_MONOMIAL ? 1 : 2)][tile][pair][sq];
}

// Argument checks of the per-component entries (`entry` names the entry in the messages).  On success bps holds the M
// descriptors and n_max the longest chunk; `empty` is set when M == 0 (nothing to do).
static int multi_args(const char *entry, int32_t M, const mlmc_basis *const *bases, int32_t K, int32_t n_levels, int32_t n_chunks,
                      const int32_t *levels, const double *const *fine, const double *const *coarse, const int64_t *n_samples,
                      bool outs, std::vector<BasisParams> &bps, int64_t &n_max, bool &empty) {
    const std::string e(entry);
    empty = false;
    if (!rt().ready) return fail("mlmc_init has not been called (no HIP device bound)");
    if (M < 0 || n_levels <= 0 || n_chunks < 0) return fail(e + ": bad M / n_levels / n_chunks");
    if (K < 1 || K > MM_MAX_K) return fail(e + ": K must be in 1..512");
    if (M == 0) {
        empty = true;
        return 0;
    }
    if (!bases || !outs || (n_chunks > 0 && (!levels || !fine || !coarse || !n_samples))) return fail(e + ": null argument");
    bps.resize(M);
    for (int m = 0; m < M; ++m) {
        const mlmc_basis *b = bases[m];
        const std::string where = e + ": component " + std::to_string(m) + ": ";
        if (!b) return fail(where + "null basis");
        if (b->out_size > 0) return fail(where + "transformed bases are not supported (pass the family member of size K)");
        const int kind = b->p.kind;
        if (kind != MLMC_LEGENDRE && kind != MLMC_MONOMIAL && kind != MLMC_FOURIER)
            return fail(where + "only Legendre, monomial and Fourier moments");
        if (kind != bases[0]->p.kind) return fail(where + "every component must use the same family");
        if (b->p.size < K) return fail(where + "basis smaller than K");
        bps[m] = b->p;
    }
    n_max = 0;
    for (int c = 0; c < n_chunks; ++c) {
        if (levels[c] < 0 || levels[c] >= n_levels) return fail(e + ": chunk level out of range");
        if (n_samples[c] < 0 || (n_samples[c] > 0 && !fine[c])) return fail(e + ": bad chunk");
        n_max = std::max(n_max, n_samples[c]);
    }
    return 0;
}

// sample blocks per (component, window) of a chunk of n samples: enough workgroups to fill the device, a few thousand
// samples each at least
static int multi_blocks(int64_t n, int64_t M, int W) {
    const int64_t want = std::max<int64_t>(1, (n + 4095) / 4096);
    const int64_t room = std::max<int64_t>(1, 4096 / (M * W));
    return (int)std::min(want, room);
}

// Both entries: the level sums (with `sq` also the sums of squares, else sums_sq_out is null and nothing of them exists) and
// the counts of every component over all chunks.
static int accum_multi(const char *entry, bool sq, int32_t M, const mlmc_basis *const *bases, int32_t K, int32_t n_levels,
                       int32_t n_chunks, const int32_t *levels, const double *const *fine, const double *const *coarse,
                       const int64_t *n_samples, int64_t *n_out, int64_t *n_rm_out, double *sums_out, double *sums_sq_out) {
    std::vector<BasisParams> bps;
    int64_t n_max = 0;
    bool empty = false;
    if (multi_args(entry, M, bases, K, n_levels, n_chunks, levels, fine, coarse, n_samples,
                   n_out && n_rm_out && sums_out && (sums_sq_out || !sq), bps, n_max, empty))
        return 1;
    if (empty) return 0;
    hipStream_t st = rt().stream;
    const int kind = bps[0].kind;
    const int tile = K <= 16 ? 0 : 1;
    const int W = (K + MV_WIN - 1) / MV_WIN;
    const int64_t L = n_levels;
    // scratch of groups of mg components (the last group may be smaller and take more sample blocks per component): table,
    // block partials (Σd, Σd², counts) and level totals, in a layout fixed for the whole call
    auto part_rows = [&](int64_t mg) {      // max over the groups of (sample blocks) x (components)
        const int64_t last = M % mg;
        int64_t r = multi_blocks(n_max, mg, W) * mg;
        if (last) r = std::max<int64_t>(r, multi_blocks(n_max, last, W) * last);
        return r;
    };
    auto sizes_for = [&](int64_t mg, size_t (&b)[7]) {
        const int64_t pr = part_rows(mg);
        b[0] = mm_align(sizeof(BasisParams) * mg);
        b[1] = mm_align(sizeof(double) * (size_t)(pr * K));
        b[2] = sq ? b[1] : 0;
        b[3] = mm_align(sizeof(int64_t) * (size_t)(pr * 2));
        b[4] = mm_align(sizeof(double) * (size_t)(L * mg * K));
        b[5] = sq ? b[4] : 0;
        b[6] = mm_align(sizeof(int64_t) * (size_t)(L * mg * 2));
        size_t t = 0;
        for (size_t v : b) t += v;
        return t;
    };
    // components in groups whose scratch stays within 64 MiB (one group up to L * M * K of about 3.5 M with the squares,
    // 7 M without)
    constexpr size_t MV_SCRATCH = size_t(64) << 20;
    size_t bsz[7];
    int64_t Mg = M;
    while (Mg > 1 && sizes_for(Mg, bsz) > MV_SCRATCH) Mg = (Mg + 1) / 2;
    static MultiWorkspace ws;
    if (ws.reserve(sizes_for(Mg, bsz))) return 1;
    char *p = ws.dev;
    BasisParams *d_tab = (BasisParams *)p;
    double *d_part = (double *)(p += bsz[0]);
    double *d_part_sq = (double *)(p += bsz[1]);
    int64_t *d_pc = (int64_t *)(p += bsz[2]);
    double *d_tot = (double *)(p += bsz[3]);
    double *d_tot_sq = (double *)(p += bsz[4]);
    int64_t *d_tc = (int64_t *)(p += bsz[5]);
    if (!sq) d_part_sq = d_tot_sq = nullptr;
    std::vector<int64_t> counts((size_t)L * M * 2);
    for (int64_t g0 = 0; g0 < M; g0 += Mg) {
        const int64_t mg = std::min<int64_t>(Mg, M - g0);
        MLMC_HIP_CHECK(hipMemcpyAsync(d_tab, bps.data() + g0, sizeof(BasisParams) * mg, hipMemcpyHostToDevice, st));
        MLMC_HIP_CHECK(hipMemsetAsync(d_tot, 0, bsz[4] + bsz[5] + bsz[6], st));
        for (int c = 0; c < n_chunks; ++c) {
            const int64_t n = n_samples[c];
            if (n == 0) continue;
            const int nb = multi_blocks(n, mg, W);
            const int lv = levels[c];
            const double *f = fine[c] + g0 * n;
            const double *co = coarse[c] ? coarse[c] + g0 * n : nullptr;
            // the first window (or the 16-term tile), then the windows after it in a launch of their own
            hipLaunchKernelGGL(multi_kernel(kind, tile, co != nullptr, sq), dim3((unsigned)nb, (unsigned)mg, 1), dim3(MM_THREADS), 0,
                               st, d_tab, f, co, n, K, nb, d_part, d_part_sq, d_pc);
            if (W > 1)
                hipLaunchKernelGGL(multi_kernel(kind, 2, co != nullptr, sq), dim3((unsigned)nb, (unsigned)mg, (unsigned)(W - 1)),
                                   dim3(MM_THREADS), 0, st, d_tab, f, co, n, K, nb, d_part, d_part_sq, d_pc);
            hipLaunchKernelGGL(sq ? k_multi_reduce<true> : k_multi_reduce<false>, dim3((unsigned)mg), dim3(MM_THREADS), 0, st, d_part,
                               d_part_sq, d_pc, K, nb, d_tot + (size_t)lv * mg * K, sq ? d_tot_sq + (size_t)lv * mg * K : nullptr,
                               d_tc + (size_t)lv * mg * 2);
            MLMC_HIP_CHECK(hipGetLastError());
        }
        // the group's rows [L][mg] into the [L][M] outputs (stream-ordered before the next group reuses the scratch)
        const size_t row = sizeof(double) * (size_t)(mg * K), ld = sizeof(double) * (size_t)M * K;
        MLMC_HIP_CHECK(hipMemcpy2DAsync(sums_out + g0 * K, ld, d_tot, row, row, (size_t)L, hipMemcpyDeviceToHost, st));
        if (sq) MLMC_HIP_CHECK(hipMemcpy2DAsync(sums_sq_out + g0 * K, ld, d_tot_sq, row, row, (size_t)L, hipMemcpyDeviceToHost, st));
        MLMC_HIP_CHECK(hipMemcpy2DAsync(counts.data() + g0 * 2, sizeof(int64_t) * (size_t)M * 2, d_tc, sizeof(int64_t) * (size_t)(mg * 2),
                                        sizeof(int64_t) * (size_t)(mg * 2), (size_t)L, hipMemcpyDeviceToHost, st));
    }
    MLMC_HIP_CHECK(wait_stream(st));
    for (int64_t l = 0; l < L; ++l)
        for (int64_t m = 0; m < M; ++m) {
            const size_t lm = (size_t)(l * M + m);
            n_out[lm] = counts[lm * 2];
            n_rm_out[lm] = counts[lm * 2 + 1];
            const std::vector<double> &sc = bases[m]->scale_c;      // Legendre: P_k = scale_c[k] q_k, P_k² = scale_c[k]² q_k²
            for (int k = 0; k < K; ++k) {
                sums_out[lm * K + k] *= sc[k];
                if (sq) sums_sq_out[lm * K + k] *= sc[k] * sc[k];
            }
        }
    return 0;
}

}  // namespace mlmc

using namespace mlmc;

extern "C" {

int mlmc_accum_estimate_multi(int32_t M, const mlmc_basis *const *bases, int32_t K, int32_t n_levels, int32_t n_chunks,
                              const int32_t *levels, const double *const *fine, const double *const *coarse,
                              const int64_t *n_samples, int64_t *n_out, int64_t *n_rm_out, double *sums_out) {
    MLMC_API_GUARD;
    return accum_multi("mlmc_accum_estimate_multi", false, M, bases, K, n_levels, n_chunks, levels, fine, coarse, n_samples, n_out,
                       n_rm_out, sums_out, nullptr);
}

int mlmc_accum_estimate_multi_var(int32_t M, const mlmc_basis *const *bases, int32_t K, int32_t n_levels, int32_t n_chunks,
                                  const int32_t *levels, const double *const *fine, const double *const *coarse,
                                  const int64_t *n_samples, int64_t *n_out, int64_t *n_rm_out, double *sums_out,
                                  double *sums_sq_out) {
    MLMC_API_GUARD;
    return accum_multi("mlmc_accum_estimate_multi_var", true, M, bases, K, n_levels, n_chunks, levels, fine, coarse, n_samples,
                       n_out, n_rm_out, sums_out, sums_sq_out);
}

}  // extern "C"
