// Aggregates of joint scenarios (gfx950): functions of the components of one scenario column -- linear forms, extremes and which
// component attains them, the number of components outside their limits -- and weighted statistics of the resulting rows.
//
// mlmc_scenario_aggregates: x [S][M][ld] -> agg [S][Q][ld_out].  One lane owns one column j of one set: it walks the M components in
// order (stride ld, so the loads of a wave are consecutive doubles of one row: coalesced for any alignment of the row) and keeps up to
// SC_NA linear accumulators, the running extremes and the count in registers; more linear rows run in further passes over x.  The
// weights and limits are read with wave-uniform indices from one small device array (scalar loads through the constant cache).  A
// value depends on its own column alone: nothing is reduced across lanes, so n, ld, S, the launch geometry and the alignment of a
// row cannot change a bit.  No atomics.
//
// mlmc_rows_weighted_sums: y [Rw][ld], weights f [ld] -> per row the counts, sum f, sum f d, sum f d^2 (d = y - c[r]) and per threshold
// sum f 1, sum f d 1.  Grid (column block, row); thread t of a block takes the columns s0 + t, s0 + t + 256, ... in order; then the wave
// butterfly, the four waves in order, and one thread per sum adds the block partials in index order.  The columns per block depend on
// n alone, so a row's bits do not depend on Rw or on its position.  Thresholds run RW_NT per pass over the row.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "device_basis.hpp"

namespace mlmc {

constexpr int SC_THREADS = 256;
constexpr int SC_NA = 8;                      // linear rows per pass over x
constexpr int SC_MAX_SETS = 65535;            // grid.y

// flags[m]: bit 0 = member of the extremes, bit 1 = has a finite limit (counts when not inside)
template <int NA, bool EX>
__global__ __launch_bounds__(SC_THREADS) void k_scenario_agg(const double *__restrict__ x, double *__restrict__ agg,
                                                             const double *__restrict__ W, const double *__restrict__ lo,
                                                             const double *__restrict__ hi, const int32_t *__restrict__ flags, int M,
                                                             int64_t n, int64_t ld, int64_t ld_out, int Q, int row0, int ex_row0,
                                                             int extras) {
    const int64_t j = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    if (j >= n) return;
    const double *xs = x + (int64_t)blockIdx.y * M * ld + j;
    double *out = agg + (int64_t)blockIdx.y * Q * ld_out + j;
    double acc[NA ? NA : 1];
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[a] = 0.0;
    double mx = 0.0, mn = 0.0;
    int amx = 0, amn = 0, cnt = 0;
    bool have = false, mx_nan = false, mn_nan = false;     // have: wave-uniform (the members are the same for every column)
    constexpr int UNROLL = EX && NA > 4 ? 2 : 4;           // the weights of an unrolled trip live in scalar registers: no spill
#pragma unroll UNROLL
    for (int m = 0; m < M; ++m) {
        const double v = xs[(int64_t)m * ld];
#pragma unroll
        for (int a = 0; a < NA; ++a) acc[a] = acc[a] + (W[(int64_t)a * M + m] * v);      // -ffp-contract=off: two roundings
        if (EX) {
            const int fl = flags[m];
            if (fl & 1) {
                const bool nan = v != v;
                if (!have) {
                    mx = mn = v;
                    amx = amn = m;
                    mx_nan = mn_nan = nan;
                    have = true;
                } else {
                    const bool up = !mx_nan && (nan || v > mx), dn = !mn_nan && (nan || v < mn);
                    mx = up ? v : mx;
                    amx = up ? m : amx;
                    mx_nan = mx_nan || (up && nan);
                    mn = dn ? v : mn;
                    amn = dn ? m : amn;
                    mn_nan = mn_nan || (dn && nan);
                }
            }
            if (fl & 2) cnt += !(lo[m] < v && v < hi[m]);
        }
    }
#pragma unroll
    for (int a = 0; a < NA; ++a) out[(int64_t)(row0 + a) * ld_out] = acc[a];
    if (EX) {
        int r = ex_row0;
        if (extras & MLMC_AGG_MAX) out[(int64_t)(r++) * ld_out] = mx;
        if (extras & MLMC_AGG_MIN) out[(int64_t)(r++) * ld_out] = mn;
        if (extras & MLMC_AGG_COUNT) out[(int64_t)(r++) * ld_out] = (double)cnt;
        if (extras & MLMC_AGG_ARGMAX) out[(int64_t)(r++) * ld_out] = (double)amx;
        if (extras & MLMC_AGG_ARGMIN) out[(int64_t)(r++) * ld_out] = (double)amn;
    }
}

template <bool EX>
static void launch_scenario_agg(int na, dim3 grid, hipStream_t st, const double *x, double *agg, const double *W, const double *lo,
                                const double *hi, const int32_t *flags, int M, int64_t n, int64_t ld, int64_t ld_out, int Q, int row0,
                                int ex_row0, int extras) {
#define MLMC_SC_CASE(NA)                                                                                                          \
    case NA:                                                                                                                      \
        hipLaunchKernelGGL((k_scenario_agg<NA, EX>), grid, dim3(SC_THREADS), 0, st, x, agg, W, lo, hi, flags, M, n, ld, ld_out, Q, \
                           row0, ex_row0, extras);                                                                                \
        break;
    switch (na) {
        MLMC_SC_CASE(0)
        MLMC_SC_CASE(1)
        MLMC_SC_CASE(2)
        MLMC_SC_CASE(3)
        MLMC_SC_CASE(4)
        MLMC_SC_CASE(5)
        MLMC_SC_CASE(6)
        MLMC_SC_CASE(7)
        MLMC_SC_CASE(8)
    }
#undef MLMC_SC_CASE
}

// ---- weighted sums of rows --------------------------------------------------------------------------------------------------
constexpr int RW_THREADS = 256;
constexpr int RW_NT = 8;                       // thresholds per pass over a row
constexpr int RW_NS = 3 + 2 * RW_NT;           // sums of a pass: sum f, sum f d, sum f d^2, then (sum f 1, sum f d 1) per threshold
constexpr int RW_MAX_BLOCKS = 1024;            // column blocks per row
constexpr int64_t RW_MIN_PER = 2048;           // columns per block at least
constexpr int RW_ROW_GROUP = 256;              // rows of one launch (block partials: 256 x 1024 x 19 doubles = 40 MB at most)

// columns per block of rows of n columns (a multiple of the block width): a function of n alone
static int64_t rw_per(int64_t n) {
    int64_t per = (n + RW_MAX_BLOCKS - 1) / RW_MAX_BLOCKS;
    per = (per + RW_THREADS - 1) / RW_THREADS * RW_THREADS;
    return std::max(per, RW_MIN_PER);
}
static int rw_blocks(int64_t n) { return (int)((n + rw_per(n) - 1) / rw_per(n)); }

// part[((r * nb) + b) * NS + k]: block b's sums of row r; pcount[(r * nb + b) * 2 + {0, 1}]: columns used / weights that are negative
// or infinite.  NT = 0: the three sums alone (no thresholds); NT = RW_NT: thresholds p0 .. p0 + RW_NT - 1 of the row (those at or
// beyond P compare against NaN: no column passes)
template <int NT>
__global__ __launch_bounds__(RW_THREADS) void k_rows_sums(const double *__restrict__ y, int64_t n, int64_t ld, const double *__restrict__ f,
                                                          const double *__restrict__ c, const double *__restrict__ t, int P, int p0,
                                                          int lower, int64_t per, int nb, double *__restrict__ part,
                                                          int64_t *__restrict__ pcount) {
    constexpr int NS = 3 + 2 * NT;
    const int b = blockIdx.x, r = blockIdx.y;
    const int64_t s0 = std::min<int64_t>(n, (int64_t)b * per), s1 = std::min<int64_t>(n, s0 + per);
    const double *row = y + (int64_t)r * ld;
    const double cr = c[r];
    double th[NT ? NT : 1];
#pragma unroll
    for (int k = 0; k < NT; ++k) th[k] = p0 + k < P ? t[(int64_t)r * P + p0 + k] : __builtin_nan("");
    double v[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) v[k] = 0.0;
    int used = 0, bad = 0;
    for (int64_t i = s0 + threadIdx.x; i < s1; i += RW_THREADS) {
        const double yi = row[i], fi = f ? f[i] : 1.0;
        const bool keep = yi == yi && fi == fi;
        used += keep;
        bad += keep && (fi < 0.0 || fi - fi != 0.0);            // fi - fi != 0: an infinite weight
        const double w = keep ? fi : 0.0, d = keep ? yi - cr : 0.0;
        const double wd = w * d;
        v[0] += w;
        v[1] += wd;
        v[2] += wd * d;
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const bool in = keep && (lower ? yi <= th[k] : yi >= th[k]);
            v[3 + 2 * k] += in ? w : 0.0;
            v[4 + 2 * k] += in ? wd : 0.0;
        }
    }
    __shared__ double red[4][NS];
    __shared__ int cred[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const double w = wave_sum(v[k]);
        if (lane == 0) red[wave][k] = w;
    }
    used = wave_sum_i(used);
    bad = wave_sum_i(bad);
    if (lane == 0) { cred[wave][0] = used; cred[wave][1] = bad; }
    __syncthreads();
    const int64_t slot = (int64_t)r * nb + b;
    if (threadIdx.x < NS) {
        const int k = threadIdx.x;
        part[slot * NS + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
    if (threadIdx.x == 64 || threadIdx.x == 65) {
        const int k = threadIdx.x - 64;
        pcount[slot * 2 + k] = ((int64_t)cred[0][k] + cred[1][k]) + ((int64_t)cred[2][k] + cred[3][k]);
    }
}

// sums[r * (3 + 2 P) + ...] and counts[r * 2 + {0, 1}] from the block partials, added in index order by one thread per sum.  The three
// row sums and the counts are written by the pass p0 = 0 alone.
template <int NT>
__global__ __launch_bounds__(64) void k_rows_merge(const double *__restrict__ part, const int64_t *__restrict__ pcount, int nb, int P, int p0,
                                                   double *__restrict__ sums, int64_t *__restrict__ counts) {
    constexpr int NS = 3 + 2 * NT;
    const int r = blockIdx.x, k = threadIdx.x;
    const int64_t W = 3 + 2 * (int64_t)P;
    if (k < NS) {
        const bool base = k < 3;
        if (base ? p0 != 0 : p0 + (k - 3) / 2 >= P) return;
        double s = 0.0;
        for (int b = 0; b < nb; ++b) s += part[((int64_t)r * nb + b) * NS + k];
        sums[r * W + (base ? k : k + 2 * p0)] = s;
    } else if (k < NS + 2 && p0 == 0) {
        int64_t s = 0;
        for (int b = 0; b < nb; ++b) s += pcount[((int64_t)r * nb + b) * 2 + (k - NS)];
        counts[(int64_t)r * 2 + (k - NS)] = s;
    }
}

// a host array's rows on the device (packed: row stride n), freed when the call returns
struct RowsUpload {
    double *p = nullptr;
    ~RowsUpload() {
        if (p) { (void)wait_stream(rt().stream); (void)hipFree(p); }
    }
    int rows(const double *src, int64_t n_rows, int64_t n, int64_t ld, hipStream_t st) {
        MLMC_HIP_CHECK(hipMalloc((void **)&p, sizeof(double) * (size_t)n_rows * (size_t)n));
        MLMC_HIP_CHECK(hipMemcpy2DAsync(p, sizeof(double) * n, src, sizeof(double) * ld, sizeof(double) * n, n_rows, hipMemcpyHostToDevice, st));
        return 0;
    }
    int space(size_t count) {
        MLMC_HIP_CHECK(hipMalloc((void **)&p, sizeof(double) * count));
        return 0;
    }
};

}  // namespace mlmc

using namespace mlmc;

extern "C" {

int mlmc_scenario_aggregates(const double *x, int64_t S, int32_t M, int64_t n, int64_t ld, const double *W, int32_t A,
                             const uint8_t *members, const double *lower, const double *upper, int32_t extras, double *agg,
                             int64_t ld_out, int mem_kind) {
    MLMC_API_GUARD;
    const std::string e("mlmc_scenario_aggregates");
    if (!rt().ready) return fail("mlmc_init has not been called (no HIP device bound)");
    if (S < 1 || M < 1 || n < 0 || A < 0)
        return fail(e + ": S = " + std::to_string(S) + ", M = " + std::to_string(M) + ", n = " + std::to_string(n) + ", A = " +
                    std::to_string(A) + " (S, M >= 1 and n, A >= 0 are required)");
    const int all = MLMC_AGG_MAX | MLMC_AGG_MIN | MLMC_AGG_COUNT | MLMC_AGG_ARGMAX | MLMC_AGG_ARGMIN;
    if (extras & ~all) return fail(e + ": unknown bits in extras");
    const int n_extra = __builtin_popcount((unsigned)extras);
    const int Q = A + n_extra;
    if ((!x && n > 0) || (!agg && Q > 0 && n > 0) || (A > 0 && !W)) return fail(e + ": null argument");      // an empty result has no address
    if (ld < n || ld_out < n) return fail(e + ": row strides ld = " + std::to_string(ld) + ", ld_out = " + std::to_string(ld_out) +
                                          " must not be below n = " + std::to_string(n));
    if (n > (int64_t(1) << 38)) return fail(e + ": more than 2^38 columns are not supported: split the columns across calls");
    if (mem_kind != MLMC_HOST && mem_kind != MLMC_DEVICE) return fail(e + ": bad mem_kind");
    for (int64_t i = 0; i < (int64_t)A * M; ++i)
        if (!std::isfinite(W[i])) return fail(e + ": the weight of row " + std::to_string(i / M) + ", component " + std::to_string(i % M) + " is not finite");
    const bool extremes = extras & (MLMC_AGG_MAX | MLMC_AGG_MIN | MLMC_AGG_ARGMAX | MLMC_AGG_ARGMIN);
    std::vector<int32_t> flags(M, 0);
    std::vector<double> lim(2 * (size_t)M);
    int n_members = 0;
    for (int m = 0; m < M; ++m) {
        if (extremes && (!members || members[m])) { flags[m] |= 1; ++n_members; }
        lim[m] = -INFINITY;
        lim[(size_t)M + m] = INFINITY;
    }
    if (extremes && n_members == 0) return fail(e + ": an extreme row is requested and no component is a member");
    if (extras & MLMC_AGG_COUNT) {
        if (!lower && !upper) return fail(e + ": the count row is requested without limits (lower and upper are both null)");
        for (int m = 0; m < M; ++m) {
            const double lo = lower ? lower[m] : -INFINITY, hi = upper ? upper[m] : INFINITY;
            if (lo != lo || hi != hi) return fail(e + ": a limit of component " + std::to_string(m) + " is NaN");
            lim[m] = lo;
            lim[(size_t)M + m] = hi;
            if (std::isfinite(lo) || std::isfinite(hi)) flags[m] |= 2;
        }
    }
    if (n == 0 || Q == 0) return 0;

    hipStream_t st = rt().stream;
    // the call's small arrays in one device buffer: W [A][M] | lower [M] | upper [M] | flags [M]
    const size_t b_w = mm_align(sizeof(double) * (size_t)A * M), b_lim = mm_align(sizeof(double) * 2 * (size_t)M);
    const size_t b_fl = mm_align(sizeof(int32_t) * (size_t)M);
    static MultiWorkspace ws;
    if (ws.reserve(b_w + b_lim + b_fl)) return 1;
    double *d_w = (double *)ws.dev, *d_lim = (double *)(ws.dev + b_w);
    int32_t *d_fl = (int32_t *)(ws.dev + b_w + b_lim);
    std::vector<char> stage(b_w + b_lim + b_fl);                    // one upload for the three
    if (A > 0) std::memcpy(stage.data(), W, sizeof(double) * (size_t)A * M);
    std::memcpy(stage.data() + b_w, lim.data(), sizeof(double) * lim.size());
    std::memcpy(stage.data() + b_w + b_lim, flags.data(), sizeof(int32_t) * flags.size());
    MLMC_HIP_CHECK(hipMemcpyAsync(ws.dev, stage.data(), stage.size(), hipMemcpyHostToDevice, st));
    const double *d_x = x;
    double *d_agg = agg;
    int64_t d_ld = ld, d_ld_out = ld_out;
    RowsUpload up_x, up_agg;
    if (mem_kind == MLMC_HOST) {
        if (up_x.rows(x, S * M, n, ld, st)) return 1;
        if (up_agg.space((size_t)S * Q * (size_t)n)) return 1;
        d_x = up_x.p;
        d_agg = up_agg.p;
        d_ld = d_ld_out = n;
    }
    const unsigned gx = (unsigned)((n + SC_THREADS - 1) / SC_THREADS);
    for (int64_t s0 = 0; s0 < S; s0 += SC_MAX_SETS) {
        const dim3 grid(gx, (unsigned)std::min<int64_t>(SC_MAX_SETS, S - s0));
        const double *xs = d_x + s0 * M * d_ld;
        double *as = d_agg + s0 * Q * d_ld_out;
        int a0 = 0;
        do {                                                        // the extra rows ride on the first pass
            const int na = std::min(SC_NA, A - a0);
            if (a0 == 0 && n_extra)
                launch_scenario_agg<true>(na, grid, st, xs, as, d_w, d_lim, d_lim + M, d_fl, M, n, d_ld, d_ld_out, Q, 0, A, extras);
            else
                launch_scenario_agg<false>(na, grid, st, xs, as, d_w + (size_t)a0 * M, d_lim, d_lim + M, d_fl, M, n, d_ld, d_ld_out, Q,
                                           a0, A, 0);
            a0 += na;
        } while (a0 < A);
        MLMC_HIP_CHECK(hipGetLastError());
    }
    if (mem_kind == MLMC_HOST)                                      // columns >= n of agg stay as they are
        MLMC_HIP_CHECK(hipMemcpy2DAsync(agg, sizeof(double) * ld_out, d_agg, sizeof(double) * n, sizeof(double) * n, (size_t)S * Q,
                                        hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(wait_stream(st));
    return 0;
}

int mlmc_rows_weighted_sums(const double *y, int64_t n_rows, int64_t n, int64_t ld, const double *f, const double *c, const double *t,
                            int32_t P, int32_t tail, int64_t *n_used, int64_t *n_skipped, double *sums, double *tail_sums,
                            int mem_kind) {
    MLMC_API_GUARD;
    const std::string e("mlmc_rows_weighted_sums");
    if (!rt().ready) return fail("mlmc_init has not been called (no HIP device bound)");
    if (n_rows < 0 || n < 0 || P < 0)
        return fail(e + ": n_rows = " + std::to_string(n_rows) + ", n = " + std::to_string(n) + ", P = " + std::to_string(P) +
                    " (none may be negative)");
    if ((!y && n_rows > 0 && n > 0) || !n_used || !n_skipped || !sums || (P > 0 && (!t || !tail_sums))) return fail(e + ": null argument");
    if (ld < n) return fail(e + ": row stride ld = " + std::to_string(ld) + " is below the row length n = " + std::to_string(n));
    if (tail != MLMC_TAIL_UPPER && tail != MLMC_TAIL_LOWER) return fail(e + ": tail must be MLMC_TAIL_UPPER or MLMC_TAIL_LOWER");
    if (mem_kind != MLMC_HOST && mem_kind != MLMC_DEVICE) return fail(e + ": bad mem_kind");
    for (int64_t i = 0; i < n_rows; ++i)
        if (c && !std::isfinite(c[i])) return fail(e + ": the centre of row " + std::to_string(i) + " is not finite");
    for (int64_t i = 0; i < n_rows * P; ++i)
        if (t[i] != t[i]) return fail(e + ": a threshold of row " + std::to_string(i / P) + " is NaN");
    for (int64_t i = 0; i < n_rows; ++i) n_used[i] = n_skipped[i] = 0;
    for (int64_t i = 0; i < n_rows * 3; ++i) sums[i] = 0.0;
    for (int64_t i = 0; i < n_rows * P * 2; ++i) tail_sums[i] = 0.0;
    if (n_rows == 0 || n == 0) return 0;

    hipStream_t st = rt().stream;
    const int nb = rw_blocks(n);
    const int64_t per = rw_per(n);
    const int64_t Rg = std::min<int64_t>(n_rows, RW_ROW_GROUP), Wd = 3 + 2 * (int64_t)P;
    // device scratch: c [Rw] | t [Rw][P] | sums [Rw][3 + 2 P] | counts [Rw][2] | block partials and counts of a row group
    const size_t b_c = mm_align(sizeof(double) * (size_t)n_rows), b_t = mm_align(sizeof(double) * (size_t)n_rows * P);
    const size_t b_s = mm_align(sizeof(double) * (size_t)n_rows * Wd), b_n = mm_align(sizeof(int64_t) * (size_t)n_rows * 2);
    const size_t b_p = mm_align(sizeof(double) * (size_t)Rg * nb * RW_NS), b_pc = mm_align(sizeof(int64_t) * (size_t)Rg * nb * 2);
    static MultiWorkspace ws;
    if (ws.reserve(b_c + b_t + b_s + b_n + b_p + b_pc)) return 1;
    char *p = ws.dev;
    double *d_c = (double *)p;
    double *d_t = (double *)(p += b_c);
    double *d_s = (double *)(p += b_t);
    int64_t *d_n = (int64_t *)(p += b_s);
    double *d_part = (double *)(p += b_n);
    int64_t *d_pc = (int64_t *)(p += b_p);
    std::vector<double> zeros;
    if (!c) zeros.assign((size_t)n_rows, 0.0);
    MLMC_HIP_CHECK(hipMemcpyAsync(d_c, c ? c : zeros.data(), sizeof(double) * (size_t)n_rows, hipMemcpyHostToDevice, st));
    if (P > 0) MLMC_HIP_CHECK(hipMemcpyAsync(d_t, t, sizeof(double) * (size_t)n_rows * P, hipMemcpyHostToDevice, st));
    const double *d_y = y, *d_f = f;
    int64_t d_ld = ld;
    RowsUpload up_y, up_f;
    if (mem_kind == MLMC_HOST) {
        if (up_y.rows(y, n_rows, n, ld, st)) return 1;
        d_y = up_y.p;
        d_ld = n;
        if (f) {
            if (up_f.rows(f, 1, n, n, st)) return 1;
            d_f = up_f.p;
        }
    }
    const int lower = tail == MLMC_TAIL_LOWER;
    for (int64_t r0 = 0; r0 < n_rows; r0 += Rg) {
        const int64_t rg = std::min<int64_t>(Rg, n_rows - r0);
        const dim3 grid((unsigned)nb, (unsigned)rg);
        const double *ys = d_y + r0 * d_ld;
        if (P == 0) {
            hipLaunchKernelGGL(k_rows_sums<0>, grid, dim3(RW_THREADS), 0, st, ys, n, d_ld, d_f, d_c + r0, d_t, 0, 0, lower, per, nb, d_part,
                               d_pc);
            hipLaunchKernelGGL(k_rows_merge<0>, dim3((unsigned)rg), dim3(64), 0, st, d_part, d_pc, nb, 0, 0, d_s + r0 * Wd, d_n + r0 * 2);
        }
        for (int p0 = 0; p0 < P; p0 += RW_NT) {
            hipLaunchKernelGGL(k_rows_sums<RW_NT>, grid, dim3(RW_THREADS), 0, st, ys, n, d_ld, d_f, d_c + r0, d_t + r0 * P, P, p0, lower,
                               per, nb, d_part, d_pc);
            hipLaunchKernelGGL(k_rows_merge<RW_NT>, dim3((unsigned)rg), dim3(64), 0, st, d_part, d_pc, nb, P, p0, d_s + r0 * Wd,
                               d_n + r0 * 2);
        }
        MLMC_HIP_CHECK(hipGetLastError());
    }
    std::vector<double> h_s((size_t)n_rows * Wd);
    std::vector<int64_t> h_n((size_t)n_rows * 2);
    MLMC_HIP_CHECK(hipMemcpyAsync(h_s.data(), d_s, sizeof(double) * h_s.size(), hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(hipMemcpyAsync(h_n.data(), d_n, sizeof(int64_t) * h_n.size(), hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(wait_stream(st));
    for (int64_t r = 0; r < n_rows; ++r)
        if (h_n[r * 2 + 1] > 0)
            return fail(e + ": " + std::to_string(h_n[r * 2 + 1]) + " weights are negative or infinite (found in row " + std::to_string(r) + ")");
    for (int64_t r = 0; r < n_rows; ++r) {
        n_used[r] = h_n[r * 2];
        n_skipped[r] = n - h_n[r * 2];
        for (int k = 0; k < 3; ++k) sums[r * 3 + k] = h_s[r * Wd + k];
        for (int64_t k = 0; k < 2 * (int64_t)P; ++k) tail_sums[r * 2 * P + k] = h_s[r * Wd + 3 + k];
    }
    return 0;
}

}  // extern "C"
