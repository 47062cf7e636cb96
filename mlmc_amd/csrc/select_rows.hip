// Percentiles of every row of a [n_rows][ld] array in one call (gfx950): the per-component domains of a vector quantity.
//
// Row m of the result is what mlmc_percentiles (select.hip) gives for row m alone, bit for bit: the same order-preserving
// key (order_key), the same two ranks and gamma per percentile and NumPy's _lerp, with every operation rounded once
// (-ffp-contract=off; q / 100 is divided on the host as in mlmc_percentiles).  Two paths, chosen by the row length n:
//   n <= RS_SORT_MAX  one workgroup per row loads the row's keys into LDS (NaNs become padding above every key), sorts them
//                     (bitonic) and reads the ranks off the sorted keys: one launch for all rows;
//   n >  RS_SORT_MAX  a segmented most-significant-digit radix select: per pass, k_rs_hist builds one 2048-bin LDS histogram
//                     per (row, distinct key prefix) and adds it into the row's global histogram; k_rs_digit (one
//                     workgroup per row, one wave per rank) picks each rank's digit on the device.  After two passes (22
//                     bits) a row whose candidates number at most RS_CAND has them collected (k_rs_collect) and sorted in LDS
//                     (k_rs_finish): three reads of the data.  Rows with heavier ties go on through all six digit passes.
// No launch and no host synchronisation depends on the data; one wait at the end of the call.  Global scratch of the radix
// path is at most RS_SCRATCH bytes: larger n_rows are processed in row groups inside the call.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "common.hpp"

namespace mlmc {
namespace {

constexpr int RS_BITS = 11;
constexpr int RS_BINS = 1 << RS_BITS;
constexpr int RS_GROUP = 4;                        // prefixes histogrammed by one workgroup (LDS: 4 x 2048 counters = 32 KiB)
constexpr int RS_MAX_Q = 32;                       // percentiles per radix round (2 ranks each); more go in further rounds
constexpr int RS_MAX_R = 2 * RS_MAX_Q;
constexpr int RS_SORT_MAX = 16384;                 // rows up to this length are sorted in LDS (128 KiB)
constexpr int RS_CAND = 8192;                      // candidates per row for the LDS finish after two digit passes (64 KiB)
constexpr size_t RS_SCRATCH = size_t(64) << 20;    // global scratch of the radix path per row group

enum { ROW_ACTIVE = 0, ROW_COLLECT = 1, ROW_DONE = 2 };

// Per-row state of the radix path, G rows of one group (scratch, see rs_layout).
struct RsState {
    unsigned int *hist;           // [G][R][RS_BINS] histograms of this pass, one per distinct prefix of the row
    unsigned long long *cand;     // [G][RS_CAND] keys under the row's 22-bit prefixes (collect path)
    unsigned long long *pref;     // [G][R] key prefix of each rank so far
    long long *k;                 // [G][R] rank left inside that prefix
    unsigned long long *upref;    // [G][R] the row's distinct prefixes, in first-occurrence order over the ranks
    double *gamma;                // [G][nq]
    int *slot;                    // [G][R] index of the rank's prefix in upref
    int *npref;                   // [G]
    int *status;                  // [G] ROW_*
    unsigned int *ccount;         // [G] candidates collected
    int R, nq;
};

__device__ __forceinline__ double key_value(unsigned long long key) {
    const unsigned long long u = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
    return __longlong_as_double((long long)u);
}

// mlmc_percentiles' plan of one percentile: virtual index (nv - 1) * q with q = percent / 100 (qf, divided on the host),
// the two neighbouring ranks and gamma.
__device__ __forceinline__ void pct_plan(int64_t nv, double qf, int64_t &prev, int64_t &next, double &g) {
    const double vi = (double)(nv - 1) * qf;
    prev = (int64_t)floor(vi);
    g = vi - (double)prev;
    if (prev < 0) { prev = 0; g = 0.0; }
    next = prev + 1;
    if (next > nv - 1) next = nv - 1;
    if (next < 0) next = 0;
}

__device__ __forceinline__ double pct_lerp(double a, double b, double g) {
    const double diff = b - a;
    double r = a + diff * g;                          // numpy.lib._function_base_impl._lerp
    if (g >= 0.5) r = b - diff * (1.0 - g);
    return r;
}

// Ascending bitonic sort of s[0, CAP) by the whole workgroup (CAP a power of two); ends with a barrier.
template <int CAP>
__device__ void block_sort(unsigned long long *s) {
    for (int k = 2; k <= CAP; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < CAP / 2; i += blockDim.x) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
                const int hi = lo + j;
                const bool up = (lo & k) == 0;
                const unsigned long long a = s[lo], b = s[hi];
                if ((a > b) == up) { s[lo] = b; s[hi] = a; }
            }
            __syncthreads();
        }
}

// ---- short rows: one workgroup sorts one row in LDS --------------------------------------------------------------------
template <int CAP>
__global__ __launch_bounds__(1024) void k_rows_sort(const double *__restrict__ x, int64_t n, int64_t ld, int64_t row0,
                                                    const double *__restrict__ qf, int nq, double *__restrict__ out,
                                                    int64_t *__restrict__ nv_out) {
    __shared__ unsigned long long s[CAP];
    __shared__ unsigned int s_nv;
    const int64_t row = row0 + blockIdx.x;
    const double *xr = x + row * ld;
    if (threadIdx.x == 0) s_nv = 0;
    __syncthreads();
    unsigned int cnt = 0;
    for (int i = threadIdx.x; i < CAP; i += blockDim.x) {
        unsigned long long key = ~0ull;               // padding and NaNs: above every non-NaN key
        if (i < n) {
            const double v = xr[i];
            if (v == v) { key = order_key(v); ++cnt; }
        }
        s[i] = key;
    }
    if (cnt) atomicAdd(&s_nv, cnt);
    __syncthreads();
    block_sort<CAP>(s);
    const int64_t nv = s_nv;
    if (threadIdx.x == 0) nv_out[row] = nv;
    if (nv == 0) return;                              // reported by the host
    for (int i = threadIdx.x; i < nq; i += blockDim.x) {
        int64_t prev, next;
        double g;
        pct_plan(nv, qf[i], prev, next, g);
        out[row * nq + i] = pct_lerp(key_value(s[prev]), key_value(s[next]), g);
    }
}

// ---- long rows: segmented radix select ---------------------------------------------------------------------------------
__device__ __forceinline__ int rs_shift(int pass) { return pass < 5 ? 53 - RS_BITS * pass : 0; }   // 53 42 31 20 9 0
__device__ __forceinline__ int rs_width(int pass) { return pass < 5 ? RS_BITS : 9; }

// Histogram of the digit of `pass` over the keys of row r under the prefixes upref[g0, g0 + RS_GROUP) (g0 = RS_GROUP *
// blockIdx.y; pass 0: all non-NaN keys into slot 0).  bpr workgroups per row, each over per_block consecutive values.
__global__ __launch_bounds__(256) void k_rs_hist(const double *__restrict__ x, int64_t n, int64_t ld, int64_t row0, int bpr,
                                                 int64_t per_block, int pass, RsState S) {
    __shared__ unsigned int lh[RS_GROUP][RS_BINS];
    const int r = blockIdx.x / bpr, part = blockIdx.x % bpr;
    if (S.status[r] != ROW_ACTIVE) return;
    const int g0 = blockIdx.y * RS_GROUP;
    const int np = pass == 0 ? (g0 == 0 ? 1 : 0) : min(RS_GROUP, S.npref[r] - g0);
    if (np <= 0) return;
    unsigned long long p[RS_GROUP];
#pragma unroll
    for (int t = 0; t < RS_GROUP; ++t) p[t] = (pass > 0 && t < np) ? S.upref[(size_t)r * S.R + g0 + t] : 0;
    for (int i = threadIdx.x; i < np * RS_BINS; i += blockDim.x) (&lh[0][0])[i] = 0;
    __syncthreads();
    const int shift = rs_shift(pass), width = rs_width(pass);
    const unsigned mask = (1u << width) - 1u;
    const double *xr = x + (row0 + r) * ld;
    const int64_t lo = (int64_t)part * per_block;
    const int64_t hi = min(n, lo + per_block);
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        const double v = xr[i];
        if (v != v) continue;
        const unsigned long long key = order_key(v);
        const unsigned digit = (unsigned)(key >> shift) & mask;
        if (pass == 0) {
            atomicAdd(&lh[0][digit], 1u);
        } else {
            const unsigned long long hk = key >> (shift + width);
#pragma unroll
            for (int t = 0; t < RS_GROUP; ++t)
                if (t < np && hk == p[t]) atomicAdd(&lh[t][digit], 1u);
        }
    }
    __syncthreads();
    unsigned int *h = S.hist + ((size_t)r * S.R + g0) * RS_BINS;
    for (int i = threadIdx.x; i < np * RS_BINS; i += blockDim.x) {
        const unsigned v = (&lh[0][0])[i];
        if (v) atomicAdd(&h[i], v);
    }
}

// The digit of every rank of row r = blockIdx.x after `pass`: one wave per rank scans the row's histogram of the rank's
// prefix.  Pass 0 first counts the valid values and plans the ranks.  Thread 0 then lists the distinct prefixes for the
// next pass, decides after pass 1 whether the row's candidates fit the LDS finish, and writes the percentiles after pass 5.
// The histograms read here are zeroed for the next pass.
__global__ __launch_bounds__(1024) void k_rs_digit(int pass, int64_t row0, RsState S, const double *__restrict__ qf,
                                                   double *__restrict__ out, int64_t *__restrict__ nv_out) {
    __shared__ unsigned long long s_pref[RS_MAX_R], s_under[RS_MAX_R], s_nv;
    __shared__ long long s_k[RS_MAX_R];
    __shared__ int s_bad;
    const int r = blockIdx.x;
    if (S.status[r] != ROW_ACTIVE) return;
    const int R = S.R, nq = S.nq;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE, n_waves = blockDim.x / WAVE;
    const int width = rs_width(pass), per_lane = (1 << width) / WAVE;
    const int used = pass == 0 ? 1 : S.npref[r];       // histogram slots filled by this pass
    unsigned int *h_row = S.hist + (size_t)r * R * RS_BINS;
    if (tid == 0) { s_nv = 0; s_bad = 0; }
    __syncthreads();
    if (pass == 0) {
        unsigned long long c = 0;
        for (int i = tid; i < RS_BINS; i += blockDim.x) c += h_row[i];
        if (c) atomicAdd(&s_nv, c);
        __syncthreads();
        const int64_t nv = (int64_t)s_nv;
        if (tid == 0) nv_out[row0 + r] = nv;
        if (nv == 0) {                                  // reported by the host
            if (tid == 0) S.status[r] = ROW_DONE;
            return;
        }
        for (int j = tid; j < R; j += blockDim.x) {
            int64_t prev, next;
            double g;
            pct_plan(nv, qf[j >> 1], prev, next, g);
            s_k[j] = (j & 1) ? next : prev;
            s_pref[j] = 0;
            if (!(j & 1)) S.gamma[(size_t)r * nq + (j >> 1)] = g;
        }
    } else {
        for (int j = tid; j < R; j += blockDim.x) {
            s_k[j] = S.k[(size_t)r * R + j];
            s_pref[j] = S.pref[(size_t)r * R + j];
        }
    }
    __syncthreads();
    for (int j = wave; j < R; j += n_waves) {
        const int sl = pass == 0 ? 0 : S.slot[(size_t)r * R + j];
        const unsigned int *h = h_row + (size_t)sl * RS_BINS + lane * per_lane;
        unsigned long long c = 0;
        for (int b = 0; b < per_lane; ++b) c += h[b];
        unsigned long long inc = c;                    // inclusive scan of the lanes' bin ranges
        for (int d = 1; d < WAVE; d <<= 1) {
            const unsigned long long t = __shfl_up(inc, d, WAVE);
            if (lane >= d) inc += t;
        }
        const unsigned long long kk = (unsigned long long)s_k[j];
        const bool mine = kk >= inc - c && kk < inc;
        if (__ballot(mine) == 0) {
            if (lane == 0) s_bad = 1;
        } else if (mine) {
            unsigned long long cum = inc - c;
            int b = 0;
            while (kk >= cum + h[b]) cum += h[b++];    // stops inside this lane's range: kk < inc
            s_k[j] = (long long)(kk - cum);
            s_pref[j] = (s_pref[j] << width) | (unsigned long long)(lane * per_lane + b);
            s_under[j] = h[b];
        }
    }
    __syncthreads();
    if (tid == 0) {
        if (s_bad) {
            nv_out[row0 + r] = -1;                      // reported by the host
            S.status[r] = ROW_DONE;
        } else {
            int np = 0;
            unsigned long long total = 0;
            for (int j = 0; j < R; ++j) {
                int u = 0;
                while (u < np && S.upref[(size_t)r * R + u] != s_pref[j]) ++u;
                if (u == np) {
                    S.upref[(size_t)r * R + np++] = s_pref[j];
                    total += s_under[j];
                }
                S.slot[(size_t)r * R + j] = u;
            }
            S.npref[r] = np;
            if (pass == 5) {                            // all 64 bits fixed: the prefixes are the keys
                for (int i = 0; i < nq; ++i)
                    out[(row0 + r) * nq + i] = pct_lerp(key_value(s_pref[2 * i]), key_value(s_pref[2 * i + 1]), S.gamma[(size_t)r * nq + i]);
                S.status[r] = ROW_DONE;
            } else if (pass == 1 && total <= (unsigned long long)RS_CAND) {
                S.ccount[r] = 0;
                S.status[r] = ROW_COLLECT;
            }
        }
    }
    for (int j = tid; j < R; j += blockDim.x) {
        S.k[(size_t)r * R + j] = s_k[j];
        S.pref[(size_t)r * R + j] = s_pref[j];
    }
    for (int i = tid; i < used * RS_BINS; i += blockDim.x) h_row[i] = 0;
}

// Rows in ROW_COLLECT: append the keys under the row's 22-bit prefixes to its candidate buffer (order irrelevant).
__global__ __launch_bounds__(256) void k_rs_collect(const double *__restrict__ x, int64_t n, int64_t ld, int64_t row0, int bpr,
                                                    int64_t per_block, RsState S) {
    __shared__ unsigned long long sp[RS_MAX_R];
    const int r = blockIdx.x / bpr, part = blockIdx.x % bpr;
    if (S.status[r] != ROW_COLLECT) return;
    const int np = S.npref[r];
    for (int i = threadIdx.x; i < np; i += blockDim.x) sp[i] = S.upref[(size_t)r * S.R + i];
    __syncthreads();
    const double *xr = x + (row0 + r) * ld;
    const int64_t lo = (int64_t)part * per_block;
    const int64_t hi = min(n, lo + per_block);
    unsigned long long *cand = S.cand + (size_t)r * RS_CAND;
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        const double v = xr[i];
        if (v != v) continue;
        const unsigned long long key = order_key(v);
        const unsigned long long hk = key >> rs_shift(1);
        bool hit = false;
        for (int t = 0; t < np; ++t) hit = hit || hk == sp[t];
        if (hit) {
            const unsigned pos = atomicAdd(&S.ccount[r], 1u);
            if (pos < RS_CAND) cand[pos] = key;
        }
    }
}

// Rows in ROW_COLLECT: sort the candidates in LDS; rank j is element k[j] of the keys under its prefix.
__global__ __launch_bounds__(1024) void k_rs_finish(int64_t row0, RsState S, double *__restrict__ out, int64_t *__restrict__ nv_out) {
    __shared__ unsigned long long s[RS_CAND];
    __shared__ unsigned long long s_val[RS_MAX_R];
    __shared__ int s_bad;
    const int r = blockIdx.x;
    if (S.status[r] != ROW_COLLECT) return;
    const int R = S.R, nq = S.nq;
    const unsigned c = S.ccount[r];
    if (threadIdx.x == 0) s_bad = c > (unsigned)RS_CAND;
    const unsigned long long *cand = S.cand + (size_t)r * RS_CAND;
    for (int i = threadIdx.x; i < RS_CAND; i += blockDim.x) s[i] = (unsigned)i < c ? cand[i] : ~0ull;
    __syncthreads();
    block_sort<RS_CAND>(s);
    const int sh = rs_shift(1);
    for (int j = threadIdx.x; j < R; j += blockDim.x) {
        const unsigned long long p = S.pref[(size_t)r * R + j], first = p << sh;
        unsigned lo = 0, hi = c < (unsigned)RS_CAND ? c : (unsigned)RS_CAND;
        const unsigned end = hi;
        while (lo < hi) {                               // first key >= p << sh
            const unsigned mid = (lo + hi) / 2;
            if (s[mid] < first) lo = mid + 1;
            else hi = mid;
        }
        const unsigned long long idx = lo + (unsigned long long)S.k[(size_t)r * R + j];
        if (idx >= end || (s[idx] >> sh) != p) s_bad = 1;
        else s_val[j] = s[idx];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_bad) {
            nv_out[row0 + r] = -1;
        } else {
            for (int i = 0; i < nq; ++i)
                out[(row0 + r) * nq + i] = pct_lerp(key_value(s_val[2 * i]), key_value(s_val[2 * i + 1]), S.gamma[(size_t)r * nq + i]);
        }
        S.status[r] = ROW_DONE;
    }
}

// Grow-only device buffers of this file (the C ABI is serialised by MLMC_API_GUARD).
struct DevPool {
    void *p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) {
            MLMC_HIP_CHECK(wait_stream(rt().stream));
            (void)hipFree(p);
            p = nullptr;
            cap = 0;
        }
        MLMC_HIP_CHECK(hipMalloc(&p, bytes));
        cap = bytes;
        return 0;
    }
};
DevPool g_io, g_scratch;

size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

// Bytes per row of the radix scratch for R ranks and nq percentiles, and the carving of G rows.
size_t rs_row_bytes(int R, int nq) {
    return (size_t)R * RS_BINS * 4 + (size_t)RS_CAND * 8 + (size_t)R * (8 + 8 + 8 + 4) + (size_t)nq * 8 + 3 * 4;
}

RsState rs_layout(char *base, int64_t G, int R, int nq) {
    RsState S;
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base + off; off += align256(bytes); return p; };
    S.hist = (unsigned int *)take((size_t)G * R * RS_BINS * 4);
    S.cand = (unsigned long long *)take((size_t)G * RS_CAND * 8);
    S.pref = (unsigned long long *)take((size_t)G * R * 8);
    S.k = (long long *)take((size_t)G * R * 8);
    S.upref = (unsigned long long *)take((size_t)G * R * 8);
    S.gamma = (double *)take((size_t)G * nq * 8);
    S.slot = (int *)take((size_t)G * R * 4);
    S.npref = (int *)take((size_t)G * 3 * 4);           // npref | status | ccount: one memset
    S.status = S.npref + G;
    S.ccount = (unsigned int *)(S.status + G);
    S.R = R;
    S.nq = nq;
    return S;
}
constexpr size_t RS_LAYOUT_SLACK = 8 * 256;              // alignment of the eight parts

int launch_rows_sort(const double *d_x, int64_t n, int64_t ld, int64_t n_rows, const double *d_qf, int nq, double *d_out,
                     int64_t *d_nv, hipStream_t st) {
    constexpr int64_t MAX_GRID = int64_t(1) << 20;
    for (int64_t row0 = 0; row0 < n_rows; row0 += MAX_GRID) {
        const unsigned g = (unsigned)std::min(MAX_GRID, n_rows - row0);
        if (n <= 256)
            hipLaunchKernelGGL(k_rows_sort<256>, dim3(g), dim3(128), 0, st, d_x, n, ld, row0, d_qf, nq, d_out, d_nv);
        else if (n <= 1024)
            hipLaunchKernelGGL(k_rows_sort<1024>, dim3(g), dim3(512), 0, st, d_x, n, ld, row0, d_qf, nq, d_out, d_nv);
        else if (n <= 4096)
            hipLaunchKernelGGL(k_rows_sort<4096>, dim3(g), dim3(1024), 0, st, d_x, n, ld, row0, d_qf, nq, d_out, d_nv);
        else
            hipLaunchKernelGGL(k_rows_sort<RS_SORT_MAX>, dim3(g), dim3(1024), 0, st, d_x, n, ld, row0, d_qf, nq, d_out, d_nv);
        MLMC_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

// Radix path for the percentiles qf[0, nq) (nq <= RS_MAX_Q) of all rows; out has row stride nq.
int launch_rows_radix(const double *d_x, int64_t n, int64_t ld, int64_t n_rows, const double *d_qf, int nq, double *d_out,
                      int64_t *d_nv, hipStream_t st) {
    const int R = 2 * nq;
    const int64_t G_max = std::max<int64_t>(1, (int64_t)((RS_SCRATCH - RS_LAYOUT_SLACK) / rs_row_bytes(R, nq)));
    const int64_t G_all = std::min(n_rows, G_max);
    if (int rc = g_scratch.reserve(RS_LAYOUT_SLACK + (size_t)G_all * rs_row_bytes(R, nq))) return rc;
    const int digit_threads = WAVE * std::min(R, 16);
    const unsigned y_groups = (unsigned)((R + RS_GROUP - 1) / RS_GROUP);
    for (int64_t row0 = 0; row0 < n_rows; row0 += G_all) {
        const int64_t G = std::min(G_all, n_rows - row0);
        RsState S = rs_layout((char *)g_scratch.p, G, R, nq);
        // workgroups per row: about four per CU in all, at least 2048 values each
        int64_t bpr = std::max<int64_t>(1, std::min<int64_t>((n + 2047) / 2048, (4 * (int64_t)rt().n_cu + G - 1) / G));
        const int64_t per_block = (n + bpr - 1) / bpr;
        bpr = (n + per_block - 1) / per_block;
        const dim3 grid_data((unsigned)(G * bpr));
        MLMC_HIP_CHECK(hipMemsetAsync(S.hist, 0, (size_t)G * R * RS_BINS * 4, st));
        MLMC_HIP_CHECK(hipMemsetAsync(S.npref, 0, (size_t)G * 3 * 4, st));
        for (int pass = 0; pass < 6; ++pass) {
            hipLaunchKernelGGL(k_rs_hist, dim3(grid_data.x, pass == 0 ? 1 : y_groups), dim3(256), 0, st, d_x, n, ld, row0, (int)bpr,
                               per_block, pass, S);
            MLMC_HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(k_rs_digit, dim3((unsigned)G), dim3(digit_threads), 0, st, pass, row0, S, d_qf, d_out, d_nv);
            MLMC_HIP_CHECK(hipGetLastError());
            if (pass == 1) {        // rows with few candidates under their 22-bit prefixes finish here
                hipLaunchKernelGGL(k_rs_collect, grid_data, dim3(256), 0, st, d_x, n, ld, row0, (int)bpr, per_block, S);
                MLMC_HIP_CHECK(hipGetLastError());
                hipLaunchKernelGGL(k_rs_finish, dim3((unsigned)G), dim3(1024), 0, st, row0, S, d_out, d_nv);
                MLMC_HIP_CHECK(hipGetLastError());
            }
        }
    }
    return 0;
}

}  // namespace
}  // namespace mlmc

using namespace mlmc;

extern "C" int mlmc_percentiles_rows(const double *x, int64_t n_rows, int64_t n, int64_t ld, const double *q_percent, int32_t nq,
                                     double *out, int64_t *n_valid, int mem_kind) {
    MLMC_API_GUARD;
    if (!rt().ready) return fail("mlmc_init has not been called (no HIP device bound)");
    if (!x || !q_percent || !out) return fail("mlmc_percentiles_rows: null argument");
    if (n_rows < 1 || n < 1)
        return fail("mlmc_percentiles_rows: n_rows = " + std::to_string(n_rows) + ", n = " + std::to_string(n) + " (both must be >= 1)");
    if (ld < n) return fail("mlmc_percentiles_rows: row stride ld = " + std::to_string(ld) + " is below the row length n = " + std::to_string(n));
    if (n > (int64_t)UINT32_MAX) return fail("mlmc_percentiles_rows: rows longer than 2^32 - 1 values are not supported");
    if (nq < 1) return fail("mlmc_percentiles_rows: nq = " + std::to_string(nq) + " (must be >= 1)");
    if (mem_kind != MLMC_HOST && mem_kind != MLMC_DEVICE) return fail("mlmc_percentiles_rows: bad mem_kind");
    for (int i = 0; i < nq; ++i)
        if (!(q_percent[i] >= 0.0 && q_percent[i] <= 100.0)) return fail("mlmc_percentiles_rows: percentiles must be in [0, 100]");
    hipStream_t st = rt().stream;
    std::vector<double> qf(nq);
    for (int i = 0; i < nq; ++i) qf[i] = q_percent[i] / 100.0;        // as mlmc_percentiles: q = percent / 100
    // one buffer for the call's small arrays: qf [nq] | out [n_rows][nq] | nv [n_rows]
    const size_t b_qf = align256(sizeof(double) * nq), b_out = align256(sizeof(double) * (size_t)n_rows * nq);
    const size_t b_nv = align256(sizeof(int64_t) * (size_t)n_rows);
    if (int rc = g_io.reserve(b_qf + b_out + b_nv)) return rc;
    double *d_qf = (double *)g_io.p;
    double *d_out = (double *)((char *)g_io.p + b_qf);
    int64_t *d_nv = (int64_t *)((char *)g_io.p + b_qf + b_out);
    const double *d_x = x;
    int64_t d_ld = ld;
    struct Upload {                                   // a host input's rows on the device, freed when the call returns
        double *p = nullptr;
        ~Upload() {
            if (p) { (void)wait_stream(rt().stream); (void)hipFree(p); }
        }
    } up;
    if (mem_kind == MLMC_HOST) {                      // packed upload of the rows (the gaps of a strided input stay behind)
        MLMC_HIP_CHECK(hipMalloc(&up.p, sizeof(double) * (size_t)n_rows * (size_t)n));
        MLMC_HIP_CHECK(hipMemcpy2DAsync(up.p, sizeof(double) * n, x, sizeof(double) * ld, sizeof(double) * n, n_rows,
                                        hipMemcpyHostToDevice, st));
        d_x = up.p;
        d_ld = n;
    }
    MLMC_HIP_CHECK(hipMemcpyAsync(d_qf, qf.data(), sizeof(double) * nq, hipMemcpyHostToDevice, st));
    if (n <= RS_SORT_MAX) {
        if (int rc = launch_rows_sort(d_x, n, d_ld, n_rows, d_qf, nq, d_out, d_nv, st)) return rc;
    } else {
        // RS_MAX_Q percentiles per round: each round selects for its slice of qf and writes a [n_rows][nqc] block of d_out,
        // the blocks are interleaved into out on the host
        for (int q0 = 0; q0 < nq; q0 += RS_MAX_Q) {
            const int nqc = std::min(RS_MAX_Q, nq - q0);
            double *d_blk = d_out + (size_t)n_rows * q0;      // [n_rows][nqc] block of this round
            if (int rc = launch_rows_radix(d_x, n, d_ld, n_rows, d_qf + q0, nqc, d_blk, d_nv, st)) return rc;
        }
    }
    std::vector<double> h_out((size_t)n_rows * nq);
    std::vector<int64_t> h_nv((size_t)n_rows);
    MLMC_HIP_CHECK(hipMemcpyAsync(h_out.data(), d_out, sizeof(double) * h_out.size(), hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(hipMemcpyAsync(h_nv.data(), d_nv, sizeof(int64_t) * h_nv.size(), hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(wait_stream(st));
    for (int64_t m = 0; m < n_rows; ++m) {
        if (h_nv[m] == 0) return fail("mlmc_percentiles_rows: row " + std::to_string(m) + " has no non-NaN value");
        if (h_nv[m] < 0) return fail("mlmc_percentiles_rows: radix select: inconsistent histogram in row " + std::to_string(m));
    }
    if (n <= RS_SORT_MAX) {
        std::copy(h_out.begin(), h_out.end(), out);
    } else {
        for (int q0 = 0; q0 < nq; q0 += RS_MAX_Q) {
            const int nqc = std::min(RS_MAX_Q, nq - q0);
            const double *blk = h_out.data() + (size_t)n_rows * q0;
            for (int64_t m = 0; m < n_rows; ++m)
                for (int i = 0; i < nqc; ++i) out[m * nq + q0 + i] = blk[m * nqc + i];
        }
    }
    if (n_valid) std::copy(h_nv.begin(), h_nv.end(), n_valid);
    return 0;
}
