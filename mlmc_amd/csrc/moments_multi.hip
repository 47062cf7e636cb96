// Per-component mean-only moment sums of a vector quantity (gfx950): M basis descriptors, ONE pass over each stored chunk.
//
// Estimate.construct_densities needs, per scalar component m, the level sums of K = linearize.extended_size(fn_m) moments of
// fn_m's family (the covariance mean by the product linearisation, the orthogonal-moments mean as T_m times the first R of
// them) -- each component masked and clipped ON ITS OWN.  The scalar chain runs two estimates per component; here one launch
// per (level, chunk) covers every component: grid (sample block, component, 32-term window), the component's BasisParams
// from a device table, the window's sums in registers, fixed-order wave / block reductions, and a fixed-order merge of the
// block partials into the level totals (k_multi_reduce), so the sums are the same bits run to run.
// Keep rule per component = the scalar path's for a one-component chunk: transform_value keeps the fine value AND (above
// level 0) the coarse value; a NaN is never kept.  The counts are therefore bit-identical to the scalar chain's.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "device_basis.hpp"

namespace mlmc {

constexpr int MM_THREADS = 256;
constexpr int MM_WIN = 32;            // terms per window (registers of one thread)
constexpr int MM_MAX_K = 512;

template <int KIND>
__device__ __forceinline__ void mm_accumulate(const BasisParams &bp, const double *__restrict__ f, const double *__restrict__ c,
                                              int64_t s0, int64_t s1, int k0, int K, double (&acc)[MM_WIN], int &kept,
                                              int &removed) {
    for (int64_t i = s0 + threadIdx.x; i < s1; i += MM_THREADS) {
        bool kf, kc = true;
        const double tf = transform_value(bp, f[i], kf);
        const double tc = c ? transform_value(bp, c[i], kc) : 0.0;
        const bool keep = kf && kc;
        kept += keep;
        removed += !keep;
        const double w = keep ? 1.0 : 0.0;      // a dropped sample yields exactly 0 in every term
        TermGen<KIND> gf, gc;
        gf.init(keep ? tf : 0.0, w, bp);
        gc.init(keep ? tc : 0.0, w, bp);
        for (int k = 0; k < k0; ++k) {          // terms before the window (the recurrences run in order)
            gf.next(k);
            if (c) gc.next(k);
        }
#pragma unroll
        for (int j = 0; j < MM_WIN; ++j) {
            const int k = k0 + j;
            if (k < K) {
                const double vf = gf.next(k);
                const double vc = c ? gc.next(k) : 0.0;
                acc[j] += vf - vc;
            }
        }
    }
}

// part[(m * nb + b) * K + k] = block b's sum of term k of component m; pcount[(m * nb + b) * 2 + {0, 1}] = kept / dropped
__global__ __launch_bounds__(MM_THREADS) void k_moments_multi(const BasisParams *__restrict__ bps, const double *__restrict__ fine,
                                                              const double *__restrict__ coarse, int64_t n, int K, int nb,
                                                              double *__restrict__ part, int64_t *__restrict__ pcount) {
    const int b = blockIdx.x, m = blockIdx.y, k0 = blockIdx.z * MM_WIN;
    const BasisParams bp = bps[m];
    const int64_t per = (n + nb - 1) / nb, s0 = std::min<int64_t>(n, (int64_t)b * per), s1 = std::min<int64_t>(n, s0 + per);
    const double *f = fine + (int64_t)m * n;
    const double *c = coarse ? coarse + (int64_t)m * n : nullptr;
    double acc[MM_WIN];
#pragma unroll
    for (int j = 0; j < MM_WIN; ++j) acc[j] = 0.0;
    int kept = 0, removed = 0;
    switch (bp.kind) {
        case MLMC_LEGENDRE: mm_accumulate<MLMC_LEGENDRE>(bp, f, c, s0, s1, k0, K, acc, kept, removed); break;
        case MLMC_MONOMIAL: mm_accumulate<MLMC_MONOMIAL>(bp, f, c, s0, s1, k0, K, acc, kept, removed); break;
        default: mm_accumulate<MLMC_FOURIER>(bp, f, c, s0, s1, k0, K, acc, kept, removed); break;
    }
    __shared__ double red[4][MM_WIN];
    __shared__ int cred[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < MM_WIN; ++j) {
        const double v = wave_sum(acc[j]);
        if (lane == 0) red[wave][j] = v;
    }
    kept = wave_sum_i(kept);
    removed = wave_sum_i(removed);
    if (lane == 0) { cred[wave][0] = kept; cred[wave][1] = removed; }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < MM_WIN && k0 + t < K) part[((int64_t)m * nb + b) * K + k0 + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    if (blockIdx.z == 0 && t < 2) pcount[((int64_t)m * nb + b) * 2 + t] = ((int64_t)cred[0][t] + cred[1][t]) + ((int64_t)cred[2][t] + cred[3][t]);
}

// tot[(m) * K + k] += sum_b part[(m * nb + b) * K + k] in block order (one workgroup per component), counts likewise
__global__ __launch_bounds__(MM_THREADS) void k_multi_reduce(const double *__restrict__ part, const int64_t *__restrict__ pcount,
                                                             int K, int nb, double *__restrict__ tot, int64_t *__restrict__ tcount) {
    const int m = blockIdx.x;
    for (int k = threadIdx.x; k < K; k += MM_THREADS) {
        double s = 0.0;
        for (int b = 0; b < nb; ++b) s += part[((int64_t)m * nb + b) * K + k];
        tot[(int64_t)m * K + k] += s;
    }
    if (threadIdx.x < 2) {
        int64_t s = 0;
        for (int b = 0; b < nb; ++b) s += pcount[((int64_t)m * nb + b) * 2 + threadIdx.x];
        tcount[(int64_t)m * 2 + threadIdx.x] += s;
    }
}

struct MultiWorkspace {
    char *dev = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        MLMC_HIP_CHECK(wait_stream(rt().stream));
        if (dev) (void)hipFree(dev);
        dev = nullptr;
        cap = 0;
        MLMC_HIP_CHECK(hipMalloc((void **)&dev, bytes));
        cap = bytes;
        return 0;
    }
};

static size_t mm_align(size_t bytes) { return (bytes + 255) / 256 * 256; }

}  // namespace mlmc

using namespace mlmc;

extern "C" {

int mlmc_accum_estimate_multi(int32_t M, const mlmc_basis *const *bases, int32_t K, int32_t n_levels, int32_t n_chunks,
                              const int32_t *levels, const double *const *fine, const double *const *coarse,
                              const int64_t *n_samples, int64_t *n_out, int64_t *n_rm_out, double *sums_out) {
    MLMC_API_GUARD;
    if (!rt().ready) return fail("mlmc_init has not been called (no HIP device bound)");
    if (M < 0 || n_levels <= 0 || n_chunks < 0) return fail("mlmc_accum_estimate_multi: bad M / n_levels / n_chunks");
    if (K < 1 || K > MM_MAX_K) return fail("mlmc_accum_estimate_multi: K must be in 1..512");
    if (M == 0) return 0;
    if (!bases || !n_out || !n_rm_out || !sums_out || (n_chunks > 0 && (!levels || !fine || !coarse || !n_samples)))
        return fail("mlmc_accum_estimate_multi: null argument");
    std::vector<BasisParams> bps(M);
    for (int m = 0; m < M; ++m) {
        const mlmc_basis *b = bases[m];
        const std::string where = "mlmc_accum_estimate_multi: component " + std::to_string(m) + ": ";
        if (!b) return fail(where + "null basis");
        if (b->out_size > 0) return fail(where + "transformed bases are not supported (pass the family member of size K)");
        const int kind = b->p.kind;
        if (kind != MLMC_LEGENDRE && kind != MLMC_MONOMIAL && kind != MLMC_FOURIER)
            return fail(where + "only Legendre, monomial and Fourier moments");
        if (kind != bases[0]->p.kind) return fail(where + "every component must use the same family");
        if (b->p.size < K) return fail(where + "basis smaller than K");
        bps[m] = b->p;
    }
    int64_t n_max = 0;
    for (int c = 0; c < n_chunks; ++c) {
        if (levels[c] < 0 || levels[c] >= n_levels) return fail("mlmc_accum_estimate_multi: chunk level out of range");
        if (n_samples[c] < 0 || (n_samples[c] > 0 && !fine[c])) return fail("mlmc_accum_estimate_multi: bad chunk");
        n_max = std::max(n_max, n_samples[c]);
    }
    hipStream_t st = rt().stream;
    const int W = (K + MM_WIN - 1) / MM_WIN;
    // sample blocks per (component, window): enough workgroups to fill the device, a few thousand samples each at least
    auto blocks_for = [&](int64_t n) {
        const int64_t want = std::max<int64_t>(1, (n + 4095) / 4096);
        const int64_t room = std::max<int64_t>(1, 4096 / ((int64_t)M * W));
        return (int)std::min(want, room);
    };
    const int nb_max = blocks_for(n_max);
    const size_t b_tab = mm_align(sizeof(BasisParams) * M), b_part = mm_align(sizeof(double) * (size_t)nb_max * M * K);
    const size_t b_pc = mm_align(sizeof(int64_t) * (size_t)nb_max * M * 2), b_tot = mm_align(sizeof(double) * (size_t)n_levels * M * K);
    const size_t b_tc = mm_align(sizeof(int64_t) * (size_t)n_levels * M * 2);
    static MultiWorkspace ws;
    if (ws.reserve(b_tab + b_part + b_pc + b_tot + b_tc)) return 1;
    BasisParams *d_tab = (BasisParams *)ws.dev;
    double *d_part = (double *)(ws.dev + b_tab);
    int64_t *d_pc = (int64_t *)(ws.dev + b_tab + b_part);
    double *d_tot = (double *)(ws.dev + b_tab + b_part + b_pc);
    int64_t *d_tc = (int64_t *)(ws.dev + b_tab + b_part + b_pc + b_tot);
    MLMC_HIP_CHECK(hipMemcpyAsync(d_tab, bps.data(), sizeof(BasisParams) * M, hipMemcpyHostToDevice, st));
    MLMC_HIP_CHECK(hipMemsetAsync(d_tot, 0, b_tot + b_tc, st));
    for (int c = 0; c < n_chunks; ++c) {
        const int64_t n = n_samples[c];
        if (n == 0) continue;
        const int nb = blocks_for(n);
        const int lv = levels[c];
        hipLaunchKernelGGL(k_moments_multi, dim3((unsigned)nb, (unsigned)M, (unsigned)W), dim3(MM_THREADS), 0, st, d_tab, fine[c],
                           coarse[c], n, K, nb, d_part, d_pc);
        hipLaunchKernelGGL(k_multi_reduce, dim3((unsigned)M), dim3(MM_THREADS), 0, st, d_part, d_pc, K, nb,
                           d_tot + (size_t)lv * M * K, d_tc + (size_t)lv * M * 2);
        MLMC_HIP_CHECK(hipGetLastError());
    }
    std::vector<int64_t> counts((size_t)n_levels * M * 2);
    MLMC_HIP_CHECK(hipMemcpyAsync(sums_out, d_tot, sizeof(double) * (size_t)n_levels * M * K, hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(hipMemcpyAsync(counts.data(), d_tc, sizeof(int64_t) * counts.size(), hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(wait_stream(st));
    for (int l = 0; l < n_levels; ++l)
        for (int m = 0; m < M; ++m) {
            const size_t lm = (size_t)l * M + m;
            n_out[lm] = counts[lm * 2];
            n_rm_out[lm] = counts[lm * 2 + 1];
            const std::vector<double> &sc = bases[m]->scale_c;      // Legendre: P_k = scale_c[k] q_k (the sums are of q_k)
            for (int k = 0; k < K; ++k) sums_out[lm * K + k] *= sc[k];
        }
    return 0;
}

}  // extern "C"
