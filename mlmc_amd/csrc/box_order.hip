// mlmc_copula_box_order_batch (include/mlmc_hip.h): Genz's variable reordering for the separation-of-variables chain of box_prob.hip
// (Genz, J. Comput. Graph. Statist. 1, 1992; Gibson, Glasbey and Elston 1994), on the device (gfx950): a greedy pivoted Cholesky
// factorisation of the covariance that integrates the component of the smallest expected conditional width first.
//
//   k_box_order : one workgroup per box, 64 ceil(M / 64) threads (one or two waves).  Thread j OWNS original component j for the whole
//                 run and never moves: its variance left v_j, its conditional mean s_j and its partial row of the factor.  perm records
//                 the positions, so no rows or columns are swapped.  The partial rows live in a workspace in global memory laid out
//                 [k][component] (M * M doubles per box, cache resident): consecutive threads read consecutive doubles.  Step i:
//                   1. every remaining thread forms a, b and the width w_j of its component (two normcdf);
//                   2. the smallest (w, original index) is found by a butterfly within the wave and two LDS slots across the waves;
//                   3. the chosen thread c stores position i, L_ii = sqrt(v_c) and its expected conditioned normal y_i; threads
//                      t < i copy L_c,t from the workspace into LDS (the row of c);
//                   4. every other remaining thread forms its new entry L_j,i from the row in LDS and its own column of the
//                      workspace, then v_j -= L_ji^2 and s_j += L_ji y_i.
//                 Three barriers per step; every loop has a trip count fixed by M and i.  At the end thread j writes row perm^-1(j)
//                 of L_out from its own workspace column.  normcdf is called through a function that is not inlined, as in
//                 box_prob.hip.  Resource figures: DESIGN.md 3.5.28.
#include <cmath>
#include <cstring>

#include "common.hpp"

namespace mlmc {

constexpr int ORDER_MAX_M = MLMC_BOX_PROB_MAX_M;
constexpr int ORDER_WAVE = 64;

__device__ __attribute__((noinline)) double order_normcdf(double x) { return normcdf(x); }
// the standard normal density; 0 at +-inf
__device__ __forceinline__ double order_normpdf(double x) { return __dmul_rn(exp(__dmul_rn(-0.5, __dmul_rn(x, x))), 0.3989422804014327); }

// the smaller of two (width, component) keys: the smaller width, ties to the lower ORIGINAL index
__device__ __forceinline__ void order_min(double &w, int &c, double w2, int c2) {
    if (w2 < w || (w2 == w && c2 < c)) w = w2, c = c2;
}

// grid (boxes); cstride = 0: one covariance for all boxes.  work [B][M][M]: the partial rows, [k][component].
__global__ __launch_bounds__(ORDER_MAX_M) void k_box_order(int M, const double *__restrict__ C, int64_t cstride, const double *__restrict__ lo,
                                                           const double *__restrict__ hi, const double *__restrict__ shift,
                                                           const int *__restrict__ first, double *work, int *__restrict__ perm,
                                                           double *__restrict__ L_out, int *__restrict__ ok) {
    __shared__ double row[ORDER_MAX_M];                // L_c,k of the chosen component, k < i
    __shared__ double red_w[2];
    __shared__ int red_c[2];
    __shared__ double pub[2];                          // L_ii, y_i
    __shared__ int bad;
    const int j = threadIdx.x, b = blockIdx.x;
    const bool own = j < M;
    const double *Cb = C + (int64_t)b * cstride;
    double *W = work + (int64_t)b * M * M;
    const double lj = own ? lo[(int64_t)b * M + j] : 0.0, hj = own ? hi[(int64_t)b * M + j] : 0.0;
    const double lt = own && shift ? __dsub_rn(lj, shift[(int64_t)b * M + j]) : lj;
    const double ht = own && shift ? __dsub_rn(hj, shift[(int64_t)b * M + j]) : hj;
    double v = own ? Cb[(int64_t)j * M + j] : 1.0, s = 0.0;
    int pos = -1;                                      // the position of this component, -1 while it remains
    const int lead = first ? first[b] : -1;
    if (j == 0) bad = 0;
    __syncthreads();
    for (int i = 0; i < M; ++i) {
        const bool remains = own && pos < 0;
        const double sd = __dsqrt_rn(v);
        const double ap = __dsub_rn(lt, s) / sd, bp = __dsub_rn(ht, s) / sd;
        const bool refl = ap > 0.0;
        const double d = order_normcdf(refl ? -bp : ap), e = order_normcdf(refl ? -ap : bp);
        const double w = lj < hj ? __dsub_rn(e, d) : 0.0;
        // a width that is NaN (a pivot that is not positive) never wins against a number
        double kw = remains && w == w ? w : HUGE_VAL;
        int kc = remains ? j : 0x7fffffff;
#pragma unroll
        for (int o = ORDER_WAVE / 2; o; o >>= 1) order_min(kw, kc, __shfl_xor(kw, o), __shfl_xor(kc, o));
        if ((j & (ORDER_WAVE - 1)) == 0) red_w[j >> 6] = kw, red_c[j >> 6] = kc;
        __syncthreads();
        kw = red_w[0], kc = red_c[0];
        if (blockDim.x > ORDER_WAVE) order_min(kw, kc, red_w[1], red_c[1]);
        // every width NaN: the lowest remaining index (the pivot check below marks the box); a forced lead takes step 0
        int c = i == 0 && lead >= 0 ? lead : kc;
        if (j == c) {
            pos = i;
            perm[(int64_t)b * M + i] = j;
            if (!(v > 0.0) || !(v < HUGE_VAL)) bad = 1;
            double y = __dsub_rn(order_normpdf(ap), order_normpdf(bp)) / w;
            if (!(w > 0.0) || !(w < HUGE_VAL) || y != y) y = ap > 0.0 ? ap : bp < 0.0 ? bp : 0.0;
            pub[0] = sd, pub[1] = y;
            W[(int64_t)i * M + j] = sd;
        }
        if (j < i) row[j] = W[(int64_t)j * M + c];
        __syncthreads();
        if (own && pos < 0) {
            const double lii = pub[0];
            double acc = 0.0;
            for (int k = 0; k < i; ++k) acc = __dadd_rn(acc, __dmul_rn(W[(int64_t)k * M + j], row[k]));
            const double lji = __dsub_rn(Cb[(int64_t)c * M + j], acc) / lii;
            W[(int64_t)i * M + j] = lji;
            v = __dsub_rn(v, __dmul_rn(lji, lji));
            s = __dadd_rn(s, __dmul_rn(lji, pub[1]));
        }
        __syncthreads();
    }
    if (own) {
        double *Lr = L_out + ((int64_t)b * M + pos) * M;
        for (int k = 0; k < M; ++k) Lr[k] = k <= pos ? W[(int64_t)k * M + j] : 0.0;
    }
    if (j == 0) ok[b] = !bad;
}

}  // namespace mlmc

using namespace mlmc;

extern "C" {

int mlmc_copula_box_order_batch(int32_t M, const double *C, int64_t cov_stride, int32_t B, const double *lo, const double *hi,
                                const double *shift, const int32_t *first, int32_t *perm, double *L_out, int32_t *ok) {
    MLMC_API_GUARD;
    const std::string e("mlmc_copula_box_order_batch");
    if (!rt().ready) return fail("mlmc_init has not been called (no HIP device bound)");
    if (M < 1) return fail(e + ": M < 1");
    if (M > ORDER_MAX_M) return fail(e + ": M = " + std::to_string(M) + " is above the cap " + std::to_string(ORDER_MAX_M));
    if (B < 1) return fail(e + ": B < 1");
    if (!C || !lo || !hi || !perm || !L_out || !ok) return fail(e + ": null argument");
    if (cov_stride != 0 && cov_stride < (int64_t)M * M)
        return fail(e + ": cov_stride = " + std::to_string(cov_stride) + " must be 0 (one shared covariance) or at least M * M = " +
                    std::to_string((int64_t)M * M));
    const int nc = cov_stride ? B : 1;
    const size_t mm = (size_t)M * M, nbx = (size_t)B * M;
    for (int g = 0; g < nc; ++g)
        for (size_t k = 0; k < mm; ++k)
            if (!std::isfinite(C[(size_t)g * (size_t)cov_stride + k]))
                return fail(e + (cov_stride ? ": box " + std::to_string(g) + ", covariance row " : ": covariance row ") + std::to_string(k / M) +
                            ": entry " + std::to_string(k % M) + " is not finite");
    for (int b = 0; b < B; ++b) {
        for (int i = 0; i < M; ++i) {
            const size_t at = (size_t)b * M + i;
            if (std::isnan(lo[at]) || std::isnan(hi[at]))
                return fail(e + ": box " + std::to_string(b) + ", component " + std::to_string(i) + ": a limit is NaN");
            if (shift && !std::isfinite(shift[at]))
                return fail(e + ": box " + std::to_string(b) + ", component " + std::to_string(i) + ": the shift is not finite");
        }
        if (first && (first[b] < -1 || first[b] >= M))
            return fail(e + ": box " + std::to_string(b) + ": first = " + std::to_string(first[b]) + " is neither -1 nor a component below M");
    }
    // what goes up: C | lo | hi | shift | first (int32); what comes down: L_out | perm | ok
    const size_t nC = (size_t)nc * mm, nsh = shift ? nbx : 0, nfi = first ? ((size_t)B + 1) / 2 : 0;
    const size_t n_in = nC + 2 * nbx + nsh + nfi;
    std::vector<double> packed(n_in);
    double *q = packed.data();
    for (int g = 0; g < nc; ++g) std::memcpy(q, C + (size_t)g * (size_t)cov_stride, sizeof(double) * mm), q += mm;
    std::memcpy(q, lo, sizeof(double) * nbx), q += nbx;
    std::memcpy(q, hi, sizeof(double) * nbx), q += nbx;
    if (nsh) std::memcpy(q, shift, sizeof(double) * nsh), q += nsh;
    if (nfi) std::memcpy(q, first, sizeof(int32_t) * (size_t)B);
    const size_t b_in = mm_align(sizeof(double) * n_in), b_work = mm_align(sizeof(double) * (size_t)B * mm), b_L = b_work;
    const size_t b_perm = mm_align(sizeof(int32_t) * nbx), b_ok = mm_align(sizeof(int32_t) * (size_t)B);
    static MultiWorkspace ws;
    if (ws.reserve(b_in + b_work + b_L + b_perm + b_ok)) return 1;
    double *d_in = (double *)ws.dev, *d_work = (double *)(ws.dev + b_in), *d_L = (double *)(ws.dev + b_in + b_work);
    int *d_perm = (int *)(ws.dev + b_in + b_work + b_L), *d_ok = (int *)(ws.dev + b_in + b_work + b_L + b_perm);
    hipStream_t st = rt().stream;
    MLMC_HIP_CHECK(hipMemcpyAsync(d_in, packed.data(), sizeof(double) * n_in, hipMemcpyHostToDevice, st));
    const double *d_C = d_in, *d_lo = d_C + nC, *d_hi = d_lo + nbx, *d_shift = nsh ? d_hi + nbx : nullptr;
    const int *d_first = nfi ? (const int *)(d_hi + nbx + nsh) : nullptr;
    const int threads = ORDER_WAVE * ((M + ORDER_WAVE - 1) / ORDER_WAVE);
    hipLaunchKernelGGL(k_box_order, dim3((unsigned)B), dim3((unsigned)threads), 0, st, (int)M, d_C, (int64_t)(cov_stride ? mm : 0), d_lo, d_hi,
                       d_shift, d_first, d_work, d_perm, d_L, d_ok);
    MLMC_HIP_CHECK(hipGetLastError());
    MLMC_HIP_CHECK(hipMemcpyAsync(L_out, d_L, sizeof(double) * (size_t)B * mm, hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(hipMemcpyAsync(perm, d_perm, sizeof(int32_t) * nbx, hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(hipMemcpyAsync(ok, d_ok, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(wait_stream(st));
    return 0;
}

}  // extern "C"
