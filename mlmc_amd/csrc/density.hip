// The max-entropy densities at points, on the device (gfx950): values, integrals, CDFs, quantiles and tail means of one problem or
// of a batch.  The arithmetic of the density is density.hpp's; this file has the kernels and the host entries.  A single entry
// (mlmc_density_eval, mlmc_density_integrate) is its batched twin at B = 1.
//
//   k_q_density   : density at the points of every problem: grid (problem, y-blocks), grid-stride over the problem's points
//   k_q_integrate : the Gauss-Legendre integral over [lo_i, hi_i], one thread per interval of the call
//
// CDFs and quantiles.  For a problem (basis, R1, lambda, sigma, [a, b]) and a rule (n_intervals, gauss_degree) the function that is
// tabulated and inverted is
//     Fhat(x) = (P_j + I(e_j, x)) / T,   x in cell j = [e_j, e_{j+1}],   e_j = a + j h, h = (b - a) / n_intervals, e_n = b,
// with C_j = the gauss_degree-point Gauss-Legendre integral of the density over cell j (density_integral), P_0 = 0,
// P_{j+1} = P_j + C_j summed in cell order, T = P_n, and I the same rule on the partial cell.
//
//   k_q_cells     : C_j of every problem, one thread per (problem, cell), into the table row [n_intervals + 1] of the problem
//   k_q_prefix    : the in-order prefix P and the mass T, one thread per problem
//   k_q_quantile  : one thread per (problem, p): binary search of p T in P, linear interpolate in the cell, then a bracketed
//                   Newton iteration on g(x) = P_j + I(e_j, x) - p T with g' = density(x); bisection whenever the step leaves
//                   the bracket or is not finite
//   k_q_cdf       : Fhat at arbitrary values, one thread per value (cell lookup + one partial-cell rule)
//   k_q_sample    : seeded draws x_j = Q(u_j) (mlmc_density_sample_batch): one workgroup per (problem, share of its draws); rule,
//                   coefficients and P row staged in LDS once, the uniform of a draw made in registers by Philox4x32-10 from
//                   (seed, stream, j), then k_q_quantile's inversion reading LDS; a lane walks its own list of draws and starts
//                   the next when its current one has ended (QInversion), so a slow draw holds up one lane, not its wave;
//                   the instances with U_IN (mlmc_density_sample_joint_batch, and with SETS mlmc_density_sample_conditional_batch)
//                   read the uniforms that copula.hip's kernels have
//                   made (u = clamp(normcdf(F z)), a Gaussian copula over the problems) instead of making them
//   k_q_scores    : normal scores normcdfinv(clamp(Fhat(x))) of stored samples (mlmc_density_scores_batch): one workgroup per
//                   (problem, run of columns) of the component-major arrays, LDS staging as k_q_sample, a lane owns the fine and
//                   the coarse value of a column as two interleaved chains of k_q_cdf's partial-cell rule
// Tail means (expected shortfall, mlmc_density_tail_means_batch): with A_j / B_j the cell sums of (t - a) rho / (b - t) rho on the
// nodes of C_j, V the forward prefix of the A_j, S and W the backward suffixes of the C_j and B_j,
//     lower(x) = a + (V_j + A(e_j, x)) / (P_j + I(e_j, x)),   upper(x) = b - (W_{j+1} + B(x, e_{j+1})) / (S_{j+1} + I(x, e_{j+1})).
//   k_q_cells<true>  : C_j (the same bits), A_j, B_j in one walk over the nodes
//   k_q_prefix<true> : P, V forwards and S, W backwards
//   k_q_tails        : one thread per (problem, x): cell lookup of k_q_cdf, then the two partial-cell rules [e_j, x] and
//                      [x, e_{j+1}] in ONE loop over the nodes, their two density evaluations interleaved term by term
// Divergences between pairs of problems (mlmc_density_divergences_batch): the rule's sums of six integrands of the two densities.
//   k_q_divergences  : one workgroup per pair; the effective coefficients of both problems go to LDS once (every lane reads the
//                      same address: a broadcast), the threads stride over the cells, two Gauss nodes advance together through
//                      the terms of p and then of q; cell sums to the pair's table row, six threads add one column each in cell order
// Expectations under a density (mlmc_density_moments_batch): the rule's sums of rho f for the terms f of a test basis, 1 and -e.
//   k_q_moments      : one workgroup per problem; steps of whole cells, lane = node fills an LDS tile [node][column] with rho f,
//                      thread = (cell, column) sums the nodes of a cell in node order, thread = column adds the cells in cell order
//                      onto a sum that stays in its register; columns beyond the tile's width follow in further chunks
// One thread owns one point from start to end, every sum has a fixed order and every loop a constant bound: a result does not
// depend on the batch, on the position of the problem in it or on the other points.  No atomics, no data-dependent launch.
// A thread of the flat-index kernels finds its problem by a binary search of its point index in the problems' offsets, so that the
// same launch geometry serves thousands of problems with a few points each and a few problems with 10^7 points each.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "copula.hpp"
#include "density.hpp"
#include "maxent_batch.hpp"
#include "sobol.hpp"

namespace mlmc {

constexpr int Q_THREADS = 256;
constexpr int Q_MAX_IT = 64;                           // iteration cap of the bracketed Newton iteration
constexpr int Q_MAX_INTERVALS = 1 << 20;
constexpr size_t Q_TABLE_BYTES = (size_t)64 << 20;     // bound of the prefix tables; more problems are processed in groups
constexpr size_t Q_JOINT_BYTES = (size_t)192 << 20;    // bound of the latent normals and copula uniforms of a joint sampling call that
                                                       // live in the workspace; more draws are processed in blocks of columns (with
                                                       // the table the workspace stays below MEB_KEEP_BYTES: it is kept between calls)
constexpr size_t Q_DIRECT_BYTES = (size_t)1 << 20;     // host point arrays beyond this are copied to the device straight from the caller's
                                                       // memory (faster from 8 MB on, measured); smaller ones ride in the block's one copy

__device__ __forceinline__ double q_integral(const QProb &P, const double *__restrict__ c, double a, double b,
                                             const double *__restrict__ nodes, const double *__restrict__ wts, int deg) {
    return with_kind(P.bp.kind, [&](auto K) { return density_integral<decltype(K)::value>(P.bp, c, P.n_coef, a, b, nodes, wts, deg); });
}

// sums of one cell [lo, hi] of the domain [a, b] in one walk over the nodes: C = the value (and the bits) of density_integral,
// A = sum w (t - a) rho, B = sum w (b - t) rho on the same nodes t and weights w
template <int KIND>
__device__ __forceinline__ void q_cell_sums(const BasisParams &bp, const double *__restrict__ c, int R, double a, double b, double lo,
                                            double hi, const double *__restrict__ nodes, const double *__restrict__ wts, int deg,
                                            double &C, double &A, double &B) {
    const double half = 0.5 * (hi - lo), mid = 0.5 * (hi + lo);
    double acc = 0.0, acc_a = 0.0, acc_b = 0.0;
    for (int k = 0; k < deg; ++k) {
        const double t = __builtin_fma(half, nodes[k], mid), w = wts[k];
        const double rho = density_value<KIND>(bp, c, R, t);
        acc = __builtin_fma(w, rho, acc);
        acc_a = __builtin_fma(w, (t - a) * rho, acc_a);
        acc_b = __builtin_fma(w, (b - t) * rho, acc_b);
    }
    C = acc * half;
    A = acc_a * half;
    B = acc_b * half;
}

// the partial-cell rules of a point x in the cell [lo, hi]: I and A on [lo, x], I and B on [x, hi], node k of both in one step
template <int KIND>
__device__ __forceinline__ void q_tail_sums(const BasisParams &bp, const double *__restrict__ c, int R, double a, double b, double lo,
                                            double x, double hi, const double *__restrict__ nodes, const double *__restrict__ wts,
                                            int deg, double &I_lo, double &A_lo, double &I_hi, double &B_hi) {
    const double half0 = 0.5 * (x - lo), mid0 = 0.5 * (x + lo), half1 = 0.5 * (hi - x), mid1 = 0.5 * (hi + x);
    double i0 = 0.0, a0 = 0.0, i1 = 0.0, b1 = 0.0;
    for (int k = 0; k < deg; ++k) {
        const double t0 = __builtin_fma(half0, nodes[k], mid0), t1 = __builtin_fma(half1, nodes[k], mid1), w = wts[k];
        double rho0, rho1;
        density_value2<KIND>(bp, c, R, t0, t1, rho0, rho1);
        i0 = __builtin_fma(w, rho0, i0);
        a0 = __builtin_fma(w, (t0 - a) * rho0, a0);
        i1 = __builtin_fma(w, rho1, i1);
        b1 = __builtin_fma(w, (b - t1) * rho1, b1);
    }
    I_lo = i0 * half0;
    A_lo = a0 * half0;
    I_hi = i1 * half1;
    B_hi = b1 * half1;
}

// cell edge j of the composite rule as an fp64 number: a + j h (two roundings, the file is compiled without contraction)
__device__ __forceinline__ double q_edge(double a, double b, double h, int nint, int j) { return j >= nint ? b : a + (double)j * h; }
__device__ __forceinline__ double q_edge(const QProb &P, double h, int nint, int j) { return q_edge(P.a, P.b, h, nint, j); }

// the cell of a value: the largest j < n with e_j <= v
__device__ __forceinline__ int q_cell_of(const QProb &P, double h, int nint, double v) {
    int lo = 0, hi = nint;
    for (int it = 0; it < 32 && hi - lo > 1; ++it) {
        const int mid = (lo + hi) >> 1;
        if (q_edge(P, h, nint, mid) <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// distance from |x| to the next larger double
__device__ __forceinline__ double q_spacing(double x) {
    const double ax = fabs(x);
    return __longlong_as_double(__double_as_longlong(ax) + 1) - ax;
}

// the problem of point `idx`: the largest k with probs[k].x_off <= idx (problems without points share their successor's offset)
__device__ __forceinline__ int q_find(const QProb *__restrict__ probs, int nprob, int64_t idx) {
    int lo = 0, hi = nprob;
    for (int it = 0; it < 32 && hi - lo > 1; ++it) {
        const int mid = (lo + hi) >> 1;
        if (probs[mid].x_off <= idx) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_q_density(const QProb *__restrict__ probs, const double *__restrict__ coef,
                                                   const double *__restrict__ x, double *__restrict__ out) {
    const QProb P = probs[blockIdx.x];
    const double *c = coef + P.c_off;
    for (int64_t i = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; i < P.n; i += (int64_t)gridDim.y * blockDim.x) {
        const double v = x[P.x_off + i];
        out[P.x_off + i] = with_kind(P.bp.kind, [&](auto K) { return density_value<decltype(K)::value>(P.bp, c, P.n_coef, v); });
    }
}

__global__ __launch_bounds__(128) void k_q_integrate(const QProb *__restrict__ probs, int nprob, int64_t npts,
                                                     const double *__restrict__ coef, const double *__restrict__ lo,
                                                     const double *__restrict__ hi, const double *__restrict__ nodes,
                                                     const double *__restrict__ wts, int deg, double *__restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npts) return;
    const QProb P = probs[q_find(probs, nprob, idx)];
    out[idx] = q_integral(P, coef + P.c_off, lo[idx], hi[idx], nodes, wts, deg);
}

// the table rows of a problem, [n + 1] doubles each, row r of problem k at tab + r * plane + k * (n + 1): the P row alone is the
// table of CDFs and quantiles, tail means have all four
enum { Q_ROW_P = 0, Q_ROW_V = 1, Q_ROW_S = 2, Q_ROW_W = 3, Q_TAIL_ROWS = 4 };

template <bool TAILS>
__global__ __launch_bounds__(128) void k_q_cells(const QProb *__restrict__ probs, int nprob, int nint, const double *__restrict__ coef,
                                                 const double *__restrict__ nodes, const double *__restrict__ wts, int deg,
                                                 double *__restrict__ tab, int64_t plane) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (int64_t)nprob * nint) return;
    const int k = (int)(gid / nint), j = (int)(gid - (int64_t)k * nint);
    const QProb P = probs[k];
    const double *c = coef + P.c_off;
    const double h = (P.b - P.a) / (double)nint;
    const double lo = q_edge(P, h, nint, j), hi = q_edge(P, h, nint, j + 1);
    double *row = tab + (int64_t)k * (nint + 1);
    if constexpr (TAILS) {
        double C, A, B;
        with_kind(P.bp.kind, [&](auto K) { q_cell_sums<decltype(K)::value>(P.bp, c, P.n_coef, P.a, P.b, lo, hi, nodes, wts, deg, C, A, B); });
        row[Q_ROW_P * plane + j + 1] = C;            // summed forwards into P_{j+1}, backwards into S_j
        row[Q_ROW_V * plane + j + 1] = A;            // summed forwards into V_{j+1}
        row[Q_ROW_W * plane + j] = B;                // summed backwards into W_j
    } else {
        row[j + 1] = q_integral(P, c, lo, hi, nodes, wts, deg);
    }
}

template <bool TAILS>
__global__ __launch_bounds__(64) void k_q_prefix(int nprob, int nint, double *__restrict__ tab, int64_t plane, const QProb *__restrict__ probs,
                                                 double *__restrict__ mass, double *__restrict__ mean) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nprob) return;
    double *row = tab + (int64_t)k * (nint + 1);
    double *__restrict__ rp = row + Q_ROW_P * plane, *__restrict__ rv = row + Q_ROW_V * plane;      // disjoint rows
    double run = 0.0, run2 = 0.0;
    if constexpr (TAILS) {
        double *__restrict__ rs = row + Q_ROW_S * plane, *__restrict__ rw = row + Q_ROW_W * plane;
        rs[nint] = 0.0;
        rw[nint] = 0.0;
        for (int j = nint - 1; j >= 0; --j) {        // from the last cell down, before the forward pass overwrites the C_j
            run += rp[j + 1];
            rs[j] = run;
            run2 += rw[j];
            rw[j] = run2;
        }
        run = 0.0;
        run2 = 0.0;
        rv[0] = 0.0;
    }
    rp[0] = 0.0;
    for (int j = 0; j < nint; ++j) {                 // P and T are the same sums with and without the tail rows
        run += rp[j + 1];
        rp[j + 1] = run;
        if constexpr (TAILS) {
            run2 += rv[j + 1];
            rv[j + 1] = run2;
        }
    }
    mass[k] = run;
    if constexpr (TAILS) mean[k] = probs[k].a + run2 / run;
}

// The inversion of one probability p as a resumable iteration, so that a lane can take its next point while its neighbours still
// iterate on theirs: begin() is the table look-up and the start in the cell, step() one evaluation of g with the bracketed Newton
// update.  The operations of a point and their order do not depend on how its steps interleave with those of other points.
template <int KIND>
struct QInversion {
    double value;                            // Q(p), once begin() or step() has returned false
    double target, ej, Pj, xl, gl, xh, gh, x, gstop;
    int it;
    // false: the value is known without iterating
    __device__ __forceinline__ bool begin(const QProb &P, const double *__restrict__ row, int nint, double p) {
        const double T = row[nint];
        value = __builtin_nan("");
        if (!(T > 0.0) || !(T < __builtin_inf())) return false;
        if (!(p >= 0.0 && p <= 1.0)) return false;
        if (p == 0.0) value = P.a;
        if (p == 1.0) value = P.b;
        if (p == 0.0 || p == 1.0) return false;
        target = p * T;
        int lo = 0, hi = nint;                  // the largest j < n with P_j <= target
        for (int k = 0; k < 32 && hi - lo > 1; ++k) {
            const int mid = (lo + hi) >> 1;
            if (row[mid] <= target) lo = mid; else hi = mid;
        }
        const int j = lo;
        const double h = (P.b - P.a) / (double)nint;
        ej = q_edge(P, h, nint, j);
        Pj = row[j];
        xl = ej;                                                           // g(xl) <= 0 <= g(xh)
        gl = Pj - target;
        xh = q_edge(P, h, nint, j + 1);
        gh = row[j + 1] - target;
        x = xl + (xh - xl) * (-gl / (gh - gl));                            // linear interpolate inside the cell
        if (!(x >= xl && x <= xh)) x = 0.5 * (xl + xh);
        gstop = 0x1p-52 * target;                                          // g is a difference of two sums near `target`: it is 0 or at least
                                                                           // about one spacing of them, nothing in between can be resolved
        it = 0;
        return true;
    }
    // false: the iteration has ended
    __device__ __forceinline__ bool step(const QProb &P, const double *__restrict__ c, const double *__restrict__ nodes,
                                         const double *__restrict__ wts, int deg) {
        const double gx = (Pj + density_integral<KIND>(P.bp, c, P.n_coef, ej, x, nodes, wts, deg)) - target;
        if (gx <= 0.0) { xl = x; gl = gx; } else { xh = x; gh = gx; }
        bool more = !(fabs(gx) <= gstop);
        if (more) {
            double xn = x - gx / density_value<KIND>(P.bp, c, P.n_coef, x);
            if (!(xn > xl && xn < xh)) xn = 0.5 * (xl + xh);                // the step left the bracket or is not finite: bisection
            more = !(fabs(xn - x) <= q_spacing(x));
            if (more) x = xn;
        }
        more = more && ++it < Q_MAX_IT;
        if (!more) value = fabs(gl) <= fabs(gh) ? xl : xh;
        return more;
    }
};

template <int KIND>
__device__ double q_invert(const QProb &P, const double *__restrict__ c, const double *__restrict__ row, int nint,
                           const double *__restrict__ nodes, const double *__restrict__ wts, int deg, double p) {
    QInversion<KIND> s;
    if (s.begin(P, row, nint, p))
        while (s.step(P, c, nodes, wts, deg)) {}
    return s.value;
}

__global__ __launch_bounds__(Q_THREADS) void k_q_quantile(const QProb *__restrict__ probs, int nprob, int nint, int64_t pt0, int64_t npts,
                                                          const double *__restrict__ coef, const double *__restrict__ tab,
                                                          const double *__restrict__ nodes, const double *__restrict__ wts, int deg,
                                                          const double *__restrict__ p, double *__restrict__ out) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= npts) return;
    const int64_t idx = pt0 + gid;
    const int k = q_find(probs, nprob, idx);
    const QProb P = probs[k];
    const double *c = coef + P.c_off, *row = tab + (int64_t)k * (nint + 1);
    const double pv = p[idx];
    out[idx] = with_kind(P.bp.kind, [&](auto K) { return q_invert<decltype(K)::value>(P, c, row, nint, nodes, wts, deg, pv); });
}

__global__ __launch_bounds__(Q_THREADS) void k_q_cdf(const QProb *__restrict__ probs, int nprob, int nint, int64_t pt0, int64_t npts,
                                                     const double *__restrict__ coef, const double *__restrict__ tab,
                                                     const double *__restrict__ nodes, const double *__restrict__ wts, int deg,
                                                     const double *__restrict__ x, double *__restrict__ out) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= npts) return;
    const int64_t idx = pt0 + gid;
    const int k = q_find(probs, nprob, idx);
    const QProb P = probs[k];
    const double *row = tab + (int64_t)k * (nint + 1);
    const double T = row[nint], v = x[idx];
    double f;
    if (!(T > 0.0) || !(T < __builtin_inf()) || v != v) {
        f = __builtin_nan("");
    } else if (v <= P.a) {
        f = 0.0;
    } else if (v >= P.b) {
        f = 1.0;
    } else {
        const double h = (P.b - P.a) / (double)nint;
        const int j = q_cell_of(P, h, nint, v);
        f = (row[j] + q_integral(P, coef + P.c_off, q_edge(P, h, nint, j), v, nodes, wts, deg)) / T;
    }
    out[idx] = f;
}

__global__ __launch_bounds__(Q_THREADS) void k_q_tails(const QProb *__restrict__ probs, int nprob, int nint, int64_t pt0, int64_t npts,
                                                       const double *__restrict__ coef, const double *__restrict__ tab, int64_t plane,
                                                       const double *__restrict__ nodes, const double *__restrict__ wts, int deg,
                                                       const double *__restrict__ x, double *__restrict__ lower, double *__restrict__ upper) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= npts) return;
    const int64_t idx = pt0 + gid;
    const int k = q_find(probs, nprob, idx);
    const QProb P = probs[k];
    const double *c = coef + P.c_off, *row = tab + (int64_t)k * (nint + 1);
    const double T = row[Q_ROW_P * plane + nint], v = x[idx];
    double lw = __builtin_nan(""), up = __builtin_nan("");
    if (T > 0.0 && T < __builtin_inf() && v == v) {
        const double h = (P.b - P.a) / (double)nint;
        const int j = q_cell_of(P, h, nint, v);
        const double ej = q_edge(P, h, nint, j), ej1 = q_edge(P, h, nint, j + 1);
        double I_lo, A_lo, I_hi, B_hi;
        with_kind(P.bp.kind, [&](auto K) {
            q_tail_sums<decltype(K)::value>(P.bp, c, P.n_coef, P.a, P.b, ej, v, ej1, nodes, wts, deg, I_lo, A_lo, I_hi, B_hi);
        });
        const double m_lo = row[Q_ROW_P * plane + j] + I_lo, m_hi = row[Q_ROW_S * plane + j + 1] + I_hi;
        // a tail without mass returns the point itself: lower(a) = a, upper(b) = b
        lw = m_lo == 0.0 ? v : P.a + (row[Q_ROW_V * plane + j] + A_lo) / m_lo;
        up = m_hi == 0.0 ? v : P.b - (row[Q_ROW_W * plane + j + 1] + B_hi) / m_hi;
    }
    lower[idx] = lw;
    upper[idx] = up;
}

// the draws of one problem of a sampling call: draws first .. first + n - 1 of stream `stream`; two doubles wide, staged as such
struct QDraw {
    int64_t first;
    uint32_t stream;
    uint32_t nan_coef;   // a coefficient of the problem is NaN: the clip of the exponent hides it from the mass, the draws are NaN
};
static_assert(sizeof(QDraw) == 2 * sizeof(double), "QDraw is staged as two doubles");

constexpr int Q_SAMPLE_THREADS = 256;                  // at most; problems with few draws get fewer waves with longer lists
constexpr int Q_SAMPLE_MAX_COEF = 512;                 // coefficients of a problem that are staged in LDS; more stay in global memory
constexpr size_t Q_SAMPLE_LDS_BYTES = 32768;           // of a workgroup: at this size the registers still bound the occupancy, not the LDS
constexpr int Q_SAMPLE_DRAWS = 32;                     // draws per lane a launch aims at: long lists even out the step counts
constexpr int Q_SAMPLE_WAVES_PER_CU = 16;              // resident waves per CU where the runtime does not tell (4 per SIMD at 123 VGPRs)

// Draws of a problem = blockIdx.x, grid-stride in y over its draws as in k_q_density.  What every draw of the problem reads is
// staged once per workgroup in LDS, Gauss nodes | weights | coefficients (COEF_LDS) | P row (ROW_LDS), and read from there by
// the inversion: every lane reads the same address in the density chain (a broadcast).  A lane walks its own list of draws and
// starts the next one as soon as its current one has ended (QInversion), whatever its neighbours are doing: a wave then takes as
// long as the lane with the largest SUM of steps, not the sum over draws of the largest step count among 64 lanes (3.5 steps
// on average, but 0.3-1.3 % of the draws take 10-50).  Neither where the values live nor how the steps interleave enters the
// arithmetic of a draw, so out is bit for bit k_q_quantile's value at the same u.
// U_IN (mlmc_density_sample_joint_batch): the uniforms are not made here but read, draw t of problem blockIdx.x from
// u_in[blockIdx.x * u_ld + t], t < u_n (a block of the call's draws, the same count for every problem); `out` points at the
// block's first draw.  seed, antithetic, u_out and the draws' first / stream are not used then.
// SETS (mlmc_density_sample_conditional_batch, with U_IN): set = blockIdx.z.  The set's uniforms are rows u_set further on in u_in
// per set and its draws x_set elements further on in out; with u_out the draw's uniform goes there too, at the draw's place.
// QMC (MLMC_SAMPLE_SOBOL): a lane's list is a RUN of consecutive draws, not every stride-th one.  The points whose indices agree
// in their low a bits share the leading a digits of every coordinate, so with a stride that is a multiple of 2^a (it always is
// one of 64) a lane would draw all its uniforms from one stratum of width 2^-a: the lanes of the tail strata would get nothing but
// slow draws and their waves would take several times as long as the others.  Consecutive points are balanced.
// Without U_IN, u_j is coordinate j of the problem's dimension of the scrambled Sobol' sequence (sobol.hpp) instead of the Philox
// uniform.  The draws' `stream` is then the row of the dimension in `sobol`, the call's table; the row's 53 words are staged in
// LDS behind the P row, a lane forms the first point of its run from the set bits of its Gray code and steps to the next with one
// XOR (the Gray codes of j - 1 and j differ in bit ctz(j)).
template <bool COEF_LDS, bool ROW_LDS, bool U_IN = false, bool SETS = false, bool QMC = false>
__global__ __launch_bounds__(Q_SAMPLE_THREADS) void k_q_sample(const QProb *__restrict__ probs, const QDraw *__restrict__ draws, int nint,
                                                               const double *__restrict__ coef, const double *__restrict__ tab,
                                                               const double *__restrict__ nodes, const double *__restrict__ wts, int deg,
                                                               uint64_t seed, int antithetic, double *__restrict__ out,
                                                               double *__restrict__ u_out, const double *__restrict__ u_in, int64_t u_ld,
                                                               int64_t u_n, int64_t u_set, int64_t x_set,
                                                               const uint64_t *__restrict__ sobol) {
    extern __shared__ double q_sample_lds[];
    static_assert(U_IN || !SETS, "the sets of a call read their uniforms");
    constexpr bool SOBOL = QMC && !U_IN;
    if constexpr (SETS) {
        out += (int64_t)blockIdx.z * x_set;
        if (u_out) u_out += (int64_t)blockIdx.z * x_set;
    }
    const QProb P = probs[blockIdx.x];
    const int64_t n_draws = U_IN ? u_n : P.n;
    const int64_t t0 = (int64_t)blockIdx.y * blockDim.x;
    const int64_t stride = (int64_t)gridDim.y * blockDim.x;
    const int64_t run = QMC ? (n_draws + stride - 1) / stride : 1;          // QMC: lane g owns the draws g run .. g run + run - 1
    if (t0 * run >= n_draws) return;                       // the whole workgroup: no draw of this problem is left for it
    const QDraw D = draws[blockIdx.x];
    double *gx = q_sample_lds, *gw = gx + deg, *cl = gw + deg, *rl = cl + (COEF_LDS ? P.n_coef : 0);
    for (int k = threadIdx.x; k < deg; k += blockDim.x) {
        gx[k] = nodes[k];
        gw[k] = wts[k];
    }
    const double *c = coef + P.c_off, *row = tab + (int64_t)blockIdx.x * (nint + 1);
    if constexpr (COEF_LDS) {
        for (int r = threadIdx.x; r < P.n_coef; r += blockDim.x) cl[r] = c[r];
        c = cl;
    }
    if constexpr (ROW_LDS) {
        for (int j = threadIdx.x; j <= nint; j += blockDim.x) rl[j] = row[j];
        row = rl;
    }
    [[maybe_unused]] uint64_t *sl = (uint64_t *)(rl + (ROW_LDS ? nint + 1 : 0));
    if constexpr (SOBOL) {
        for (int k = threadIdx.x; k < SOBOL_ROW; k += blockDim.x) sl[k] = sobol[(int64_t)D.stream * SOBOL_ROW + k];
    }
    __syncthreads();
    with_kind(P.bp.kind, [&](auto K) {
        QInversion<decltype(K)::value> s;
        bool busy = false;
        int64_t cur = 0;                                    // the draw `s` iterates on
        int64_t t = (t0 + threadIdx.x) * run;
        const int64_t step = QMC ? 1 : stride, t_end = QMC ? std::min(t + run, n_draws) : n_draws;
        [[maybe_unused]] const int64_t t_first = t;
        [[maybe_unused]] uint64_t point = 0;                // SOBOL: m of the lane's last point
        // U_IN: the uniform of the lane's next draw is loaded while it inverts the one before, so that no wave waits for memory
        // at the start of a draw
        [[maybe_unused]] const double *ur = nullptr;
        [[maybe_unused]] double u_next = 0.0;
        if constexpr (U_IN) {
            ur = u_in + ((SETS ? (int64_t)blockIdx.z * u_set : 0) + (int64_t)blockIdx.x) * u_ld;
            if (t < t_end) u_next = ur[t];
        }
        while (busy || t < t_end) {
            if (!busy) {                                    // this lane's next draw, while other lanes go on with theirs
                double u;
                if constexpr (U_IN) {
                    u = u_next;
                    if (t + step < t_end) u_next = ur[t + step];
                    if constexpr (SETS) {
                        if (u_out) u_out[P.x_off + t] = u;
                    }
                } else if constexpr (SOBOL) {
                    const uint64_t j = (uint64_t)(D.first + t);
                    point = t == t_first ? sobol_point(sl, j) : point ^ sl[__builtin_ctzll(j)];
                    u = sobol_unit(point);
                    if (u_out) u_out[P.x_off + t] = u;
                } else {
                    const uint64_t j = (uint64_t)(D.first + t);
                    u = q_uniform(seed, D.stream, antithetic ? j >> 1 : j);
                    if (antithetic && (j & 1)) u = 1.0 - u;
                    if (u_out) u_out[P.x_off + t] = u;
                }
                busy = !D.nan_coef && s.begin(P, row, nint, u);
                if (!busy) out[P.x_off + t] = D.nan_coef ? __builtin_nan("") : s.value;
                cur = t;
                t += step;
            }
            if (busy && !s.step(P, c, gx, gw, deg)) {
                out[P.x_off + cur] = s.value;
                busy = false;
            }
        }
    });
}

constexpr int Q_SCORE_THREADS = 256;

// Normal scores z = normcdfinv(clamp(Fhat(x))) of stored samples (mlmc_density_scores_batch): problem = blockIdx.x = row of the
// component-major arrays, blockIdx.y = a run of columns from c0 on.  LDS as in k_q_sample: Gauss nodes | weights | coefficients
// (COEF_LDS) | P row (ROW_LDS), staged once per workgroup and read as broadcasts.  A lane owns TWO values and walks their
// partial-cell rules as two interleaved chains (density_integral2), so one chain's latency hides behind the other's: with a
// coarse array the fine and the coarse value of its column, without one the fine values of its column and of the column one
// workgroup width further on.  Consecutive lanes take consecutive columns of a row: loads and stores are coalesced.  Every kept
// value costs one partial-cell rule, so there are no lane lists; a value that is not kept rides along at x = a and is discarded.
// The kernel has no loop over columns: normcdfinv sits behind the integrals' loop nest, not inside a loop that would keep its
// constants in registers (copula.hip).  The arithmetic of u is k_q_cdf's (q_cell_of, q_edge, density_integral's chain): the same bits.
template <bool COEF_LDS, bool ROW_LDS>
__global__ __launch_bounds__(Q_SCORE_THREADS) void k_q_scores(const QProb *__restrict__ probs, const QDraw *__restrict__ draws, int nint,
                                                              const double *__restrict__ coef, const double *__restrict__ tab,
                                                              const double *__restrict__ nodes, const double *__restrict__ wts, int deg,
                                                              const double *__restrict__ fine, const double *__restrict__ coarse,
                                                              int64_t c0, int64_t n, int64_t ld_in, double *__restrict__ z_fine,
                                                              double *__restrict__ z_coarse, int64_t ld_out, double *__restrict__ u_fine,
                                                              double *__restrict__ u_coarse) {
    extern __shared__ __attribute__((aligned(16))) double q_score_lds[];
    const QProb P = probs[blockIdx.x];
    double *gx = q_score_lds, *gw = gx + deg, *cl = gw + deg, *rl = cl + (COEF_LDS ? P.n_coef : 0);
    for (int k = threadIdx.x; k < deg; k += blockDim.x) {
        gx[k] = nodes[k];
        gw[k] = wts[k];
    }
    const double *c = coef + P.c_off, *row = tab + (int64_t)blockIdx.x * (nint + 1);
    if constexpr (COEF_LDS) {
        for (int r = threadIdx.x; r < P.n_coef; r += blockDim.x) cl[r] = c[r];
        c = cl;
    }
    if constexpr (ROW_LDS) {
        for (int j = threadIdx.x; j <= nint; j += blockDim.x) rl[j] = row[j];
        row = rl;
    }
    __syncthreads();
    const bool pair = coarse != nullptr;
    const int64_t t0 = c0 + (int64_t)blockIdx.y * (pair ? 1 : 2) * blockDim.x + threadIdx.x, t1 = pair ? t0 : t0 + blockDim.x;
    if (t0 >= n) return;
    const bool have1 = t1 < n;
    const int64_t in_row = (int64_t)blockIdx.x * ld_in, out_row = (int64_t)blockIdx.x * ld_out;
    const double v0 = fine[in_row + t0], v1 = have1 ? (pair ? coarse : fine)[in_row + t1] : __builtin_nan("");
    const double T = row[nint];
    const bool ok = T > 0.0 && T < __builtin_inf() && !draws[blockIdx.x].nan_coef;
    const bool keep0 = ok && v0 > P.a && v0 < P.b, keep1 = ok && v1 > P.a && v1 < P.b;      // false for NaN
    const double x0 = keep0 ? v0 : P.a, x1 = keep1 ? v1 : P.a;
    const double h = (P.b - P.a) / (double)nint;
    const int j0 = q_cell_of(P, h, nint, x0), j1 = q_cell_of(P, h, nint, x1);
    double i0, i1;
    with_kind(P.bp.kind, [&](auto K) {
        density_integral2<decltype(K)::value>(P.bp, c, P.n_coef, q_edge(P, h, nint, j0), x0, q_edge(P, h, nint, j1), x1, gx, gw, deg, i0, i1);
    });
    const double u0 = keep0 ? (row[j0] + i0) / T : __builtin_nan(""), u1 = keep1 ? (row[j1] + i1) / T : __builtin_nan("");
    // a u that is NaN (the density left its basis' domain) stays NaN: fmax would turn it into the clamp's end
    const double s0 = normcdfinv(fmin(fmax(u0, 0x1p-53), 1.0 - 0x1p-53)), s1 = normcdfinv(fmin(fmax(u1, 0x1p-53), 1.0 - 0x1p-53));
    z_fine[out_row + t0] = u0 == u0 ? s0 : u0;
    if (u_fine) u_fine[out_row + t0] = u0;
    if (have1) {
        (pair ? z_coarse : z_fine)[out_row + t1] = u1 == u1 ? s1 : u1;
        double *u_second = pair ? u_coarse : u_fine;
        if (u_second) u_second[out_row + t1] = u1;
    }
}

// one pair of a divergences call: problems `first` (p) and `second` (q) on [lo, hi]; three doubles wide, staged as such
struct QPair {
    double lo, hi;
    int32_t first, second;
};
static_assert(sizeof(QPair) == 3 * sizeof(double), "QPair is staged as three doubles");

constexpr int Q_DIV_THREADS = 256;                     // at most; a launch has as many waves as the rule has cells to fill

// node (t, w) of a pair into the six sums, each one FMA: every integrand from rho_p and d = e_q - e_p alone
__device__ __forceinline__ void q_div_node(double w, double ep, double rp, double eq, double rq, double (&acc)[MLMC_DIV_COUNT]) {
    const double d = eq - ep, x = expm1(d), y = expm1(0.5 * d);
    acc[MLMC_DIV_KL] = __builtin_fma(w, rp * (x - d), acc[MLMC_DIV_KL]);
    acc[MLMC_DIV_L2SQ] = __builtin_fma(w, (rp * rp) * (x * x), acc[MLMC_DIV_L2SQ]);
    acc[MLMC_DIV_TV] = __builtin_fma(w, (0.5 * rp) * fabs(x), acc[MLMC_DIV_TV]);
    acc[MLMC_DIV_H2] = __builtin_fma(w, (0.5 * rp) * (y * y), acc[MLMC_DIV_H2]);
    acc[MLMC_DIV_MASS_P] = __builtin_fma(w, rp, acc[MLMC_DIV_MASS_P]);
    acc[MLMC_DIV_MASS_Q] = __builtin_fma(w, rq, acc[MLMC_DIV_MASS_Q]);
}

// nodes k .. k + N - 1 of a cell: N chains through the terms of p, then N through those of q (the two may be of different families)
template <int N>
__device__ __forceinline__ void q_div_nodes(const QProb &Pp, const double *__restrict__ cp, const QProb &Pq, const double *__restrict__ cq,
                                            double half, double mid, const double *__restrict__ nodes, const double *__restrict__ wts, int k,
                                            double (&acc)[MLMC_DIV_COUNT], bool &ok) {
    double t[N], ep[N], rp[N], eq[N], rq[N];
#pragma unroll
    for (int i = 0; i < N; ++i) t[i] = __builtin_fma(half, nodes[k + i], mid);
    with_kind(Pp.bp.kind, [&](auto K) { density_exponents<decltype(K)::value, N>(Pp.bp, cp, Pp.n_coef, t, ep, rp, ok); });
    with_kind(Pq.bp.kind, [&](auto K) { density_exponents<decltype(K)::value, N>(Pq.bp, cq, Pq.n_coef, t, eq, rq, ok); });
#pragma unroll
    for (int i = 0; i < N; ++i) q_div_node(wts[k + i], ep[i], rp[i], eq[i], rq[i], acc);
}

// tab: row of pair g of the launch at tab + g * MLMC_DIV_COUNT * nint, column c of cell j at [c * nint + j]; LDS: the coefficients
// of p, then those of q
__global__ __launch_bounds__(Q_DIV_THREADS) void k_q_divergences(const QProb *__restrict__ probs, const QPair *__restrict__ pairs, int nint,
                                                                 const double *__restrict__ coef, const double *__restrict__ nodes,
                                                                 const double *__restrict__ wts, int deg, double *__restrict__ tab,
                                                                 double *__restrict__ out) {
    extern __shared__ double q_div_coef[];
    const QPair pr = pairs[blockIdx.x];
    const QProb Pp = probs[pr.first], Pq = probs[pr.second];
    double *cp = q_div_coef, *cq = q_div_coef + Pp.n_coef;
    for (int r = threadIdx.x; r < Pp.n_coef; r += blockDim.x) cp[r] = coef[Pp.c_off + r];
    for (int r = threadIdx.x; r < Pq.n_coef; r += blockDim.x) cq[r] = coef[Pq.c_off + r];
    __syncthreads();
    double *row = tab + (int64_t)blockIdx.x * MLMC_DIV_COUNT * nint;
    const double h = (pr.hi - pr.lo) / (double)nint;
    for (int j = threadIdx.x; j < nint; j += blockDim.x) {
        const double lo = q_edge(pr.lo, pr.hi, h, nint, j), hi = q_edge(pr.lo, pr.hi, h, nint, j + 1);
        const double half = 0.5 * (hi - lo), mid = 0.5 * (hi + lo);              // density_integral's
        double acc[MLMC_DIV_COUNT] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        bool ok = true;
        int k = 0;
        for (; k + 1 < deg; k += 2) q_div_nodes<2>(Pp, cp, Pq, cq, half, mid, nodes, wts, k, acc, ok);
        if (k < deg) q_div_nodes<1>(Pp, cp, Pq, cq, half, mid, nodes, wts, k, acc, ok);
#pragma unroll
        for (int c = 0; c < MLMC_DIV_COUNT; ++c) row[(int64_t)c * nint + j] = ok ? acc[c] * half : __builtin_nan("");
    }
    __syncthreads();
    if (threadIdx.x < MLMC_DIV_COUNT) {
        const double *col = row + (int64_t)threadIdx.x * nint;
        double run = 0.0;
        for (int j = 0; j < nint; ++j) run += col[j];
        out[(int64_t)blockIdx.x * MLMC_DIV_COUNT + threadIdx.x] = run;
    }
}

// the test basis of one problem of a moments call; nine doubles wide, staged as such
struct QTest {
    BasisParams bp;
    int32_t S;          // underlying terms q_0 .. q_{S-1}; the columns of the problem are these, then 1, then -e
    int32_t reserved;
};
static_assert(sizeof(QTest) == 9 * sizeof(double), "QTest is staged as nine doubles");

constexpr int Q_MOM_THREADS = 256;
constexpr int Q_MOM_MAX_TERMS = 512;
constexpr int Q_MOM_SUMS = (Q_MOM_MAX_TERMS + 2 + Q_MOM_THREADS - 1) / Q_MOM_THREADS;      // running column sums of a thread
constexpr size_t Q_MOM_LDS_BYTES = 65536;

// LDS of a moments launch, in doubles: coefficients [coef_cap] | tile [cps * deg][stride] | cell sums [cps][chunk].  A step takes
// `cps` whole cells, wave w the cells w * cpw .. of the step (cpw = max(1, 64 / deg) cells, lane = node); the columns go through
// the tile `chunk` at a time (stride = chunk | 1: odd, so that the lanes of a wave writing one column hit different banks)
struct QMomLayout {
    int coef_cap, cpw, cps, chunk, stride;
};

// Expectations under the density of one problem (mlmc_density_moments_batch): column sums of rho f over the rule.
//   phase 1, thread = node : the density chain, then the test generator in term order; rho f into the tile
//   phase 2a, thread = (cell, column) : C_j[f] = (sum_k fma(w_k, tile, acc)) * half in node order, into the cell sums
//   phase 2b, thread = column : the cells of the step in cell order onto the running sum in the thread's register
// The generator of a node stays in its thread's registers from one chunk of columns to the next.
template <int TKIND>
__device__ __forceinline__ void q_mom_problem(const QProb &P, const QTest &T, const double *__restrict__ c, double *__restrict__ tile,
                                              double *__restrict__ cell_sums, int *__restrict__ flags, int nint,
                                              const double *__restrict__ nodes, const double *__restrict__ wts, int deg,
                                              const QMomLayout &L, double (&sum)[Q_MOM_SUMS]) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int cw = lane / deg, k = lane - cw * deg;                 // cell within the wave, node within the cell
    const int cs = wave * L.cpw + cw;                               // cell within the step
    const int n_col = T.S + 2;
    const double h = (P.b - P.a) / (double)nint;
    for (int j0 = 0; j0 < nint; j0 += L.cps) {
        const int nc = min(L.cps, nint - j0);
        const bool active = cw < L.cpw && cs < nc;
        TermGen<TKIND> g;
        double rho = 0.0, neg_e = 0.0;
        if (active) {
            const double lo = q_edge(P, h, nint, j0 + cs), hi = q_edge(P, h, nint, j0 + cs + 1);
            const double half = 0.5 * (hi - lo), mid = 0.5 * (hi + lo);          // density_integral's
            const double t = __builtin_fma(half, nodes[k], mid);
            bool ok = true;
            with_kind(P.bp.kind, [&](auto K) {
                DensityChain<decltype(K)::value> ch;
                ch.begin(P.bp, t);
                for (int r = 0; r < P.n_coef; ++r) ch.term(r, c[r]);
                rho = ch.value();
                neg_e = -ch.exponent();
                ok = ch.valid();
            });
            if (!ok) flags[0] = 1;
            bool keep;
            const double tt = transform_value(T.bp, t, keep);
            if (!keep) flags[1] = 1;
            g.init(keep ? tt : 0.0, 1.0, T.bp);
        }
        for (int c0 = 0; c0 < n_col; c0 += L.chunk) {
            const int ncc = min(L.chunk, n_col - c0);
            if (active) {
                double *row = tile + (size_t)(cs * deg + k) * L.stride;
                for (int i = 0; i < ncc; ++i) {
                    const int r = c0 + i;
                    row[i] = r < T.S ? rho * g.next(r) : (r == T.S ? rho : rho * neg_e);
                }
            }
            __syncthreads();
            for (int p = tid; p < nc * ncc; p += blockDim.x) {
                const int cell = p / ncc, i = p - cell * ncc;
                const double lo = q_edge(P, h, nint, j0 + cell), hi = q_edge(P, h, nint, j0 + cell + 1);
                const double half = 0.5 * (hi - lo);
                const double *col = tile + (size_t)cell * deg * L.stride + i;
                double acc = 0.0;
                for (int kk = 0; kk < deg; ++kk) acc = __builtin_fma(wts[kk], col[(size_t)kk * L.stride], acc);
                cell_sums[cell * L.chunk + i] = acc * half;
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < Q_MOM_SUMS; ++s) {
                const int i = tid + s * Q_MOM_THREADS - c0;
                if (i >= 0 && i < ncc)
                    for (int cell = 0; cell < nc; ++cell) sum[s] += cell_sums[cell * L.chunk + i];
            }
            // the next writes of the cell sums come after the next barrier, those of the tile after the one above
        }
    }
}

// out: row of problem g of the launch at out + g * ldo: the sums of the columns q_0 .. q_{S-1}, 1, -e
__global__ __launch_bounds__(Q_MOM_THREADS) void k_q_moments(const QProb *__restrict__ probs, const QTest *__restrict__ tests, int nint,
                                                             const double *__restrict__ coef, const double *__restrict__ nodes,
                                                             const double *__restrict__ wts, int deg, QMomLayout L, int ldo,
                                                             double *__restrict__ out) {
    extern __shared__ double q_mom_lds[];
    __shared__ int flags[2];                 // a node where the density chain is not valid / that the test basis does not keep
    const QProb P = probs[blockIdx.x];
    const QTest T = tests[blockIdx.x];
    double *c = q_mom_lds, *tile = c + L.coef_cap, *cell_sums = tile + (size_t)L.cps * deg * L.stride;
    for (int r = threadIdx.x; r < P.n_coef; r += blockDim.x) c[r] = coef[P.c_off + r];
    if (threadIdx.x < 2) flags[threadIdx.x] = 0;
    __syncthreads();
    double sum[Q_MOM_SUMS];
#pragma unroll
    for (int s = 0; s < Q_MOM_SUMS; ++s) sum[s] = 0.0;
    with_kind(T.bp.kind, [&](auto K) { q_mom_problem<decltype(K)::value>(P, T, c, tile, cell_sums, flags, nint, nodes, wts, deg, L, sum); });
    __syncthreads();
    const bool bad_density = flags[0] != 0, bad_test = flags[1] != 0;
#pragma unroll
    for (int s = 0; s < Q_MOM_SUMS; ++s) {
        const int col = threadIdx.x + s * Q_MOM_THREADS;
        if (col < T.S + 2) out[(int64_t)blockIdx.x * ldo + col] = (bad_density || (bad_test && col < T.S)) ? __builtin_nan("") : sum[s];
    }
}

// HIP-event time of the point kernels (k_q_quantile / k_q_cdf / k_q_sample; k_q_quantile + k_q_tails of a tail-means call as one), for
// mlmc_density_quantiles_kernel_time: one event pair per timed span of a call (begin() .. end() around the point kernels of a group
// or block), read by collect() after the call's own wait.  Best effort: the timing never fails a call, a span whose events cannot
// be made or recorded is not counted.
struct QTiming {
    std::vector<hipEvent_t> ev;
    double ms = 0.0;
    int64_t launches = 0;
    size_t timed = 0;                 // recorded spans of the running call
    bool open = false;                // the running span has its first event
    void begin(hipStream_t st) {
        open = false;
        while (ev.size() < 2 * (timed + 1)) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return;
            ev.push_back(e);
        }
        open = hipEventRecord(ev[2 * timed], st) == hipSuccess;
    }
    void end(hipStream_t st) {
        if (open && hipEventRecord(ev[2 * timed + 1], st) == hipSuccess) ++timed;
        open = false;
    }
    void collect() {
        for (size_t k = 0; k < timed; ++k) {
            float span = 0.0f;
            if (hipEventElapsedTime(&span, ev[2 * k], ev[2 * k + 1]) != hipSuccess) continue;
            ms += span;
            ++launches;
        }
        timed = 0;
    }
};
static QTiming &q_timing() {
    static QTiming t;
    return t;
}
// the timing of a new call: no spans yet, whatever an earlier call that failed has left
static QTiming &q_call_timing() {
    QTiming &t = q_timing();
    t.timed = 0;
    return t;
}

// validated problems of a call: table, effective coefficients, point offsets
struct QSetup {
    std::vector<QProb> probs;
    std::vector<double> coef;
    int64_t n_tot = 0;
};

// the message of problem i; a single entry has one problem and does not name it
static int q_fail(const char *fn, bool single, int i, const std::string &what) {
    return single ? fail(std::string(fn) + ": " + what) : meb_fail(fn, i, what);
}

// a and b: the domains, or both NULL for an entry that takes none
static int q_prepare(const char *fn, bool single, int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                     const double *sigma, const double *a, const double *b, const int64_t *n, QSetup &S) {
    int ldv = 0;
    for (int i = 0; i < B; ++i) {
        const mlmc_basis *bs = bases[i];
        if (!bs) return q_fail(fn, single, i, "null basis");
        const int max_out = bs->out_size > 0 ? bs->out_size : bs->p.size;
        if (R1[i] <= 0 || R1[i] > max_out) return q_fail(fn, single, i, "R1 out of range");
        if (bs->p.kind != MLMC_LEGENDRE && bs->p.kind != MLMC_MONOMIAL && bs->p.kind != MLMC_FOURIER && bs->p.kind != MLMC_SPLINE)
            return q_fail(fn, single, i, "unsupported basis kind");
        if (n[i] < 0) return q_fail(fn, single, i, "n < 0");
        if (a && !(std::isfinite(a[i]) && std::isfinite(b[i]) && a[i] < b[i]))
            return q_fail(fn, single, i, "the domain must be finite with a < b");
        ldv = std::max(ldv, (int)R1[i]);
    }
    S.probs.resize(B);
    for (int i = 0; i < B; ++i) {
        const mlmc_basis *bs = bases[i];
        const std::vector<double> c = effective_coeffs(bs, lambda + (size_t)i * ldv, sigma + (size_t)i * ldv, R1[i]);
        const int Reff = bs->out_size > 0 ? bs->p.size : R1[i];
        QProb &p = S.probs[i];
        p.bp = bs->p;
        p.n_coef = Reff;
        p.c_off = (int64_t)S.coef.size();
        p.x_off = S.n_tot;
        p.n = n[i];
        p.a = a ? a[i] : 0.0;
        p.b = a ? b[i] : 0.0;
        S.coef.insert(S.coef.end(), c.begin(), c.begin() + Reff);
        S.n_tot += n[i];
    }
    return 0;
}

// One call's block in the shared workspace (meb_ws), every part 256-byte aligned:
//   pinned buffer and device, at the same offsets:  problem table | coefficients | Gauss nodes | Gauss weights | staged point arrays
//   behind them, device only:  the call's further arrays (outputs, tables);   pinned buffer only:  results on their way back
// q_stage lays the block out, reserves it and fills in table, coefficients and rule; upload() sends it with the caller's host
// points: in the block's one copy, or (`direct`: no pinned room for them) each array straight from the caller's memory.
struct QBlock {
    const QProb *probs;               // device
    const double *coef, *gx, *gw;     // device
    double *h_in[2], *d_in[2];        // staged point arrays: pinned and device side
    double *d[7];                     // device only
    double *h[1];                     // pinned only
    size_t head_bytes, in_bytes;      // up to the end of the Gauss rule / of the staged arrays
    bool direct;
    int upload(std::initializer_list<const double *> points, size_t len) const {
        hipStream_t st = rt().stream;
        int i = 0;
        for (const double *src : points) {
            if (len > 0 && direct) MLMC_HIP_CHECK(hipMemcpyAsync(d_in[i], src, sizeof(double) * len, hipMemcpyHostToDevice, st));
            if (len > 0 && !direct) std::memcpy(h_in[i], src, sizeof(double) * len);
            ++i;
        }
        MLMC_HIP_CHECK(hipMemcpyAsync(meb_ws().dev, meb_ws().host, direct ? head_bytes : in_bytes, hipMemcpyHostToDevice, st));
        return 0;
    }
};

// array lengths in doubles (0: an array the call does not need); deg = 0: no Gauss rule
static int q_stage(const QSetup &S, int deg, std::initializer_list<size_t> staged, std::initializer_list<size_t> dev_only,
                   std::initializer_list<size_t> host_only, QBlock &K) {
    std::vector<double> gx, gw;
    gauss_legendre(deg, gx, gw);
    const void *src[4] = {S.probs.data(), S.coef.data(), gx.data(), gw.data()};
    const size_t bytes[4] = {sizeof(QProb) * S.probs.size(), sizeof(double) * S.coef.size(), sizeof(double) * deg, sizeof(double) * deg};
    size_t at[4], head = 0;
    for (int k = 0; k < 4; ++k) {
        at[k] = head;
        head += meb_align(bytes[k]);
    }
    const auto span = [](std::initializer_list<size_t> lens) {
        size_t sum = 0;
        for (size_t len : lens) sum += meb_align(sizeof(double) * len);
        return sum;
    };
    K.head_bytes = head;
    K.in_bytes = head + span(staged);
    K.direct = K.in_bytes - head > Q_DIRECT_BYTES;
    const size_t host_in = K.direct ? head : K.in_bytes;
    MebWorkspace &ws = meb_ws();
    if (ws.reserve(K.in_bytes + span(dev_only), host_in + span(host_only))) return 1;
    for (int k = 0; k < 4; ++k)
        if (bytes[k]) std::memcpy(ws.host + at[k], src[k], bytes[k]);
    K.probs = (const QProb *)(ws.dev + at[0]);
    K.coef = (const double *)(ws.dev + at[1]);
    K.gx = (const double *)(ws.dev + at[2]);
    K.gw = (const double *)(ws.dev + at[3]);
    const auto carve = [](char *base, size_t from, std::initializer_list<size_t> lens, double **ptr) {
        for (size_t len : lens) {
            *ptr++ = (double *)(base + from);
            from += meb_align(sizeof(double) * len);
        }
    };
    carve(ws.host, head, staged, K.h_in);
    carve(ws.dev, head, staged, K.d_in);
    carve(ws.dev, K.in_bytes, dev_only, K.d);
    carve(ws.host, host_in, host_only, K.h);
    return 0;
}

// The head of an entry: the bound device, the count of problems (named `count` in the message) and the arguments every call needs
// (`args`: all of them given).  0: go on; 1: failed; -1: a call without problems, which is no error and does nothing.
static int q_head(const char *fn, const char *count, int32_t B, bool args) {
    if (!rt().ready) return fail("mlmc_init has not been called (no HIP device bound)");
    if (B < 0) return fail(std::string(fn) + ": " + count + " < 0");
    if (B == 0) return -1;
    if (!args) return fail(std::string(fn) + ": null argument");
    return 0;
}

// The rule of an entry: the cells nint and the Gauss degree deg from the arguments and their zero defaults; mem_kind is checked
// behind them for the entries that take one
static int q_rule(const char *fn, int32_t n_intervals, int32_t gauss_degree, int &nint, int &deg, int mem_kind = MLMC_HOST) {
    if (n_intervals < 0 || n_intervals > Q_MAX_INTERVALS) return fail(std::string(fn) + ": n_intervals must be in 0..1048576 (0 = 64)");
    if (gauss_degree < 0 || gauss_degree > 64) return fail(std::string(fn) + ": gauss_degree must be in 0..64 (0 = 21)");
    if (mem_kind != MLMC_HOST && mem_kind != MLMC_DEVICE) return fail(std::string(fn) + ": bad mem_kind");
    nint = n_intervals > 0 ? n_intervals : 64;
    deg = gauss_degree > 0 ? gauss_degree : 21;
    return 0;
}

// The groups of the table bound: `count` problems with `rows` table rows of nint + 1 entries each run G at a time, and a row of
// the group's table is `plane` entries from the next
struct QGroups {
    int G;
    int64_t plane;
};
static QGroups q_groups(int count, size_t rows, int nint) {
    const int G = (int)std::min<size_t>((size_t)count, std::max<size_t>(1, Q_TABLE_BYTES / (sizeof(double) * rows * ((size_t)nint + 1))));
    return QGroups{G, (int64_t)G * (nint + 1)};
}

// The tables of the np_g problems from g0 (tails: with the rows of the tail means), in stream order behind whatever read the
// table of the group before: the cell integrals and their prefix, which leaves the masses at d_mass and, tails, the means at d_mean
static void q_tables(hipStream_t st, bool tails, const QBlock &K, int g0, int np_g, int nint, int deg, double *d_tab, int64_t plane,
                     double *d_mass, double *d_mean) {
    const auto cells = tails ? k_q_cells<true> : k_q_cells<false>;
    const auto prefix = tails ? k_q_prefix<true> : k_q_prefix<false>;
    const int64_t n_cells = (int64_t)np_g * nint;
    hipLaunchKernelGGL(cells, dim3((unsigned)((n_cells + 127) / 128)), dim3(128), 0, st, K.probs + g0, np_g, nint, K.coef, K.gx, K.gw, deg,
                       d_tab, plane);
    hipLaunchKernelGGL(prefix, dim3((unsigned)((np_g + 63) / 64)), dim3(64), 0, st, np_g, nint, d_tab, plane, K.probs + g0, d_mass, d_mean);
}

// The one staged array of a call that sends more than doubles: the parts one after another, each from a whole double on.  add()
// copies a part in (src NULL: zeros) and hands back where it starts; at() is its place on the device once q_stage has laid out
// the block and upload() has sent `data`.
struct QPack {
    std::vector<double> data;
    template <class T>
    size_t add(const T *src, size_t count) {
        const size_t at = data.size();
        data.resize(at + (sizeof(T) * count + sizeof(double) - 1) / sizeof(double));
        if (src && count) std::memcpy(data.data() + at, src, sizeof(T) * count);
        return at;
    }
    template <class T>
    const T *at(const QBlock &K, size_t part) const {
        return (const T *)(K.d_in[0] + part);
    }
};

// mlmc_density_eval (single; x and out in host or device memory) and mlmc_density_eval_batch
static int q_eval(const char *fn, bool single, int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                  const double *sigma, const double *x, const int64_t *n, double *out, int mem_kind) {
    if (const int r = q_head(fn, "B", B, bases && R1 && lambda && sigma && n)) return r > 0;
    QSetup S;
    if (q_prepare(fn, single, B, bases, R1, lambda, sigma, nullptr, nullptr, n, S)) return 1;
    if (S.n_tot == 0) return 0;
    if (!x || !out) return fail(std::string(fn) + ": null argument");
    hipStream_t st = rt().stream;
    const bool stage = mem_kind == MLMC_HOST;            // device arrays are used in place
    const size_t np = stage ? (size_t)S.n_tot : 0;
    QBlock K;
    if (q_stage(S, 0, {np}, {np}, {}, K)) return 1;
    if (K.upload({x}, np)) return 1;
    double *d_out = stage ? K.d[0] : out;
    int64_t n_max = 0;
    for (const QProb &p : S.probs) n_max = std::max(n_max, p.n);
    const unsigned gy = (unsigned)std::min<int64_t>((n_max + 255) / 256, 1024);
    hipLaunchKernelGGL(k_q_density, dim3((unsigned)B, gy), dim3(256), 0, st, K.probs, K.coef, stage ? (const double *)K.d_in[0] : x, d_out);
    MLMC_HIP_CHECK(hipGetLastError());
    if (stage) MLMC_HIP_CHECK(hipMemcpyAsync(out, d_out, sizeof(double) * np, hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(wait_stream(st));
    meb_ws().trim(MEB_KEEP_BYTES);
    return 0;
}

// mlmc_density_integrate (single) and mlmc_density_integrate_batch
static int q_integrate(const char *fn, bool single, int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                       const double *sigma, const double *lo, const double *hi, const int64_t *n, int32_t degree, double *out) {
    if (const int r = q_head(fn, "B", B, bases && R1 && lambda && sigma && n)) return r > 0;
    if (degree <= 0 || degree > 64) return fail(std::string(fn) + ": degree must be in 1..64");
    QSetup S;
    if (q_prepare(fn, single, B, bases, R1, lambda, sigma, nullptr, nullptr, n, S)) return 1;
    if (S.n_tot == 0) return 0;
    if (!lo || !hi || !out) return fail(std::string(fn) + ": null argument");
    hipStream_t st = rt().stream;
    const size_t np = (size_t)S.n_tot;
    QBlock K;
    if (q_stage(S, degree, {np, np}, {np}, {}, K)) return 1;
    if (K.upload({lo, hi}, np)) return 1;
    hipLaunchKernelGGL(k_q_integrate, dim3((unsigned)((S.n_tot + 127) / 128)), dim3(128), 0, st, K.probs, (int)B, S.n_tot, K.coef,
                       (const double *)K.d_in[0], (const double *)K.d_in[1], K.gx, K.gw, (int)degree, K.d[0]);
    MLMC_HIP_CHECK(hipGetLastError());
    MLMC_HIP_CHECK(hipMemcpyAsync(out, K.d[0], sizeof(double) * np, hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(wait_stream(st));
    meb_ws().trim(MEB_KEEP_BYTES);
    return 0;
}

enum QMode { Q_CDF, Q_QUANTILES, Q_TAILS, Q_SAMPLE };

// what a sampling call has instead of points
struct QSampling {
    uint64_t seed;
    const uint32_t *streams;          // [B] host or NULL
    const int64_t *first;             // [B] host or NULL
    int32_t flags;
    double *u_out;                    // may be NULL
};

// the flags of a sampling call
static int q_sample_flags(const char *fn, int32_t flags) {
    if (flags & ~(MLMC_SAMPLE_ANTITHETIC | MLMC_SAMPLE_SOBOL)) return fail(std::string(fn) + ": unknown flag bits");
    if ((flags & MLMC_SAMPLE_ANTITHETIC) && (flags & MLMC_SAMPLE_SOBOL))
        return fail(std::string(fn) + ": MLMC_SAMPLE_SOBOL and MLMC_SAMPLE_ANTITHETIC exclude each other");
    return 0;
}

// The draws table of the problems of a call, as every entry with k_q_sample or k_q_scores stages it: the nan_coef flag of each
// problem, first = 0 and the problem's index as its stream.  The entries whose uniforms come from elsewhere read the flag alone.
static std::vector<QDraw> q_draw_table(const QSetup &S) {
    std::vector<QDraw> draws(S.probs.size());
    for (size_t i = 0; i < S.probs.size(); ++i) {
        const double *c = S.coef.data() + S.probs[i].c_off;
        const bool nan_coef = std::any_of(c, c + S.probs[i].n_coef, [](double v) { return v != v; });
        draws[i] = QDraw{0, (uint32_t)i, nan_coef ? 1u : 0u};
    }
    return draws;
}

// first draw and stream of every problem of mlmc_density_sample_batch, into its draws table
static int q_draws(const char *fn, const QSetup &S, const QSampling &smp, std::vector<QDraw> &draws) {
    for (size_t i = 0; i < S.probs.size(); ++i) {
        const QProb &p = S.probs[i];
        const int64_t first = smp.first ? smp.first[i] : 0;
        if (first < 0) return meb_fail(fn, (int)i, "first < 0");
        if (first > INT64_MAX - p.n) return meb_fail(fn, (int)i, "first + n overflows int64");
        if ((smp.flags & MLMC_SAMPLE_SOBOL) && first + p.n > SOBOL_MAX_INDEX)
            return meb_fail(fn, (int)i, "first + n is beyond the 2^52 points of the Sobol' sequence");
        draws[i].first = first;
        if (smp.streams) draws[i].stream = smp.streams[i];
    }
    return 0;
}

// A sampling launch: the kernel's instance and its LDS (the rule, the coefficients and the P row, each as far as it fits), and
// the resident waves per CU of that instance as the runtime reports them for its registers and this LDS size.
using QSampler = decltype(&k_q_sample<true, true, false>);
struct QSampleLaunch {
    QSampler kernel = nullptr;
    size_t lds_bytes = 0;
    int64_t waves_per_cu = Q_SAMPLE_WAVES_PER_CU;
    // Launch geometry (no draw depends on it) of npts draws in all, at most n_max of one problem.  The draws are dealt to the chip's
    // wave slots in k rounds, k such that a lane's list has about Q_SAMPLE_DRAWS draws, or one round of shorter lists when there
    // are too few draws for that: a problem gets as many waves (first within a workgroup, then workgroups) as its lists of that
    // length need.
    void geometry(int64_t npts, int64_t n_max, unsigned &threads, unsigned &gy) const {
        const int64_t lanes = 64 * waves_per_cu * std::max(1, rt().n_cu);
        const int64_t rounds = std::max<int64_t>(1, (npts + lanes * Q_SAMPLE_DRAWS / 2) / (lanes * Q_SAMPLE_DRAWS));
        const int64_t list = std::max<int64_t>(1, npts / (lanes * rounds));
        const int64_t th = 64 * std::clamp<int64_t>(n_max / (64 * list), 1, Q_SAMPLE_THREADS / 64);
        threads = (unsigned)th;
        gy = (unsigned)std::clamp<int64_t>((n_max + th * list / 2) / (th * list), 1, 65535);
    }
};
// What a workgroup of k_q_sample / k_q_scores stages in LDS for the problems of a call: the rule always, the coefficients if every
// problem has at most Q_SAMPLE_MAX_COEF, and then the P row if all of it fits into Q_SAMPLE_LDS_BYTES; `extra` bytes go on top
// (the Sobol' row of a problem's dimension)
struct QLdsPlan {
    bool coef_lds, row_lds;
    size_t bytes;
};
static QLdsPlan q_lds_plan(const QSetup &S, int nint, int deg, size_t extra = 0) {
    int max_coef = 0;
    for (const QProb &p : S.probs) max_coef = std::max(max_coef, p.n_coef);
    const bool coef_lds = max_coef <= Q_SAMPLE_MAX_COEF;
    const size_t lds_head = sizeof(double) * (2 * (size_t)deg + (coef_lds ? max_coef : 0)) + extra, lds_row = sizeof(double) * ((size_t)nint + 1);
    const bool row_lds = coef_lds && lds_head + lds_row <= Q_SAMPLE_LDS_BYTES;
    return QLdsPlan{coef_lds, row_lds, lds_head + (row_lds ? lds_row : 0)};
}

// u_in: the instance that reads its uniforms (mlmc_density_sample_joint_batch); sets: the one that reads them per set
// (mlmc_density_sample_conditional_batch); qmc: the instances of MLMC_SAMPLE_SOBOL, whose lanes own runs of draws and which, in
// mlmc_density_sample_batch, make Sobol' uniforms
template <bool U_IN, bool SETS, bool QMC>
static QSampler q_sampler(const QLdsPlan &plan) {
    return plan.row_lds    ? k_q_sample<true, true, U_IN, SETS, QMC>
           : plan.coef_lds ? k_q_sample<true, false, U_IN, SETS, QMC>
                           : k_q_sample<false, false, U_IN, SETS, QMC>;
}
static QSampleLaunch q_sample_launch(const QSetup &S, int nint, int deg, bool u_in, bool sets = false, bool qmc = false) {
    const QLdsPlan plan = q_lds_plan(S, nint, deg, qmc && !u_in ? sizeof(uint64_t) * SOBOL_ROW : 0);
    QSampleLaunch L;
    if (qmc && sets) L.kernel = q_sampler<true, true, true>(plan);
    else if (qmc && u_in) L.kernel = q_sampler<true, false, true>(plan);
    else if (qmc) L.kernel = q_sampler<false, false, true>(plan);
    else if (sets) L.kernel = q_sampler<true, true, false>(plan);
    else if (u_in) L.kernel = q_sampler<true, false, false>(plan);
    else L.kernel = q_sampler<false, false, false>(plan);
    L.lds_bytes = plan.bytes;
    int resident = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, L.kernel, Q_SAMPLE_THREADS, L.lds_bytes) == hipSuccess && resident > 0)
        L.waves_per_cu = (int64_t)resident * (Q_SAMPLE_THREADS / 64);
    return L;
}

// mlmc_density_cdf_batch (Q_CDF), mlmc_density_quantiles_batch (Q_QUANTILES), mlmc_density_tail_means_batch (Q_TAILS: `out`
// receives the quantiles, lower_out / upper_out the tail means at them, mean_out the problems' means; all NULL otherwise) and
// mlmc_density_sample_batch (Q_SAMPLE: no points x, `smp` instead; `out` receives the draws, smp->u_out their uniforms)
static int q_on_rule(const char *fn, QMode mode, int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                     const double *sigma, const double *a, const double *b, int32_t n_intervals, int32_t gauss_degree,
                     const double *x, const int64_t *n, double *out, double *mass_out, int mem_kind, double *lower_out = nullptr,
                     double *upper_out = nullptr, double *mean_out = nullptr, const QSampling *smp = nullptr) {
    if (const int r = q_head(fn, "B", B, bases && R1 && lambda && sigma && a && b && n)) return r > 0;
    int nint, deg;
    if (q_rule(fn, n_intervals, gauss_degree, nint, deg, mem_kind)) return 1;
    const bool tails = mode == Q_TAILS, sample = mode == Q_SAMPLE;
    if (sample && q_sample_flags(fn, smp->flags)) return 1;
    const bool sobol = sample && (smp->flags & MLMC_SAMPLE_SOBOL);
    QSetup S;
    if (q_prepare(fn, false, B, bases, R1, lambda, sigma, a, b, n, S)) return 1;
    std::vector<QDraw> draws;
    if (sample) draws = q_draw_table(S);
    if (sample && q_draws(fn, S, *smp, draws)) return 1;
    // MLMC_SAMPLE_SOBOL: the rows of the call's distinct dimensions; a problem's draws entry names its row instead of its stream
    std::vector<uint64_t> sobol_tab;
    if (sobol) {
        std::vector<uint32_t> slot;
        if (sobol_call_table(fn, "problem", smp->seed, smp->streams, B, sobol_tab, slot)) return 1;
        for (int i = 0; i < B; ++i) draws[i].stream = slot[i];
    }
    if (S.n_tot > 0 && ((!sample && !x) || !out || (tails && (!lower_out || !upper_out)))) return fail(std::string(fn) + ": null argument");
    if (S.n_tot == 0 && !mass_out && !mean_out) return 0;
    hipStream_t st = rt().stream;
    const bool stage = mem_kind == MLMC_HOST && S.n_tot > 0;
    const size_t rows = tails ? Q_TAIL_ROWS : 1;                             // table rows per problem
    const auto [G, plane] = q_groups(B, rows, nint);
    const size_t np = stage ? (size_t)S.n_tot : 0, nm = (size_t)B * (tails ? 2 : 1);      // staged points; masses, then means
    // what goes up with the block: the points, or of a sampling call the draws table | the Sobol' table (uint64); a sampling call
    // returns the uniforms in the place of the lower tail means
    QPack pack;
    pack.add(draws.data(), draws.size());
    const size_t at_sobol = pack.add(sobol_tab.data(), sobol_tab.size());
    const size_t n_in = sample ? pack.data.size() : np;
    if (sample) lower_out = smp->u_out;
    QBlock K;
    if (q_stage(S, deg, {n_in}, {nm, rows * (size_t)plane, np, lower_out ? np : 0, tails ? np : 0}, {nm}, K)) return 1;
    if (K.upload({sample ? pack.data.data() : x}, n_in)) return 1;
    double *d_mass = K.d[0], *d_mean = d_mass + B, *d_tab = K.d[1];
    const double *d_x = stage ? K.d_in[0] : x;
    double *d_out = stage ? K.d[2] : out, *d_lower = stage && lower_out ? K.d[3] : lower_out, *d_upper = stage ? K.d[4] : upper_out;
    QSampleLaunch L;
    if (sample) L = q_sample_launch(S, nint, deg, false, false, sobol);
    QTiming &tm = q_call_timing();
    for (int g0 = 0; g0 < B; g0 += G) {
        const int np_g = std::min(G, B - g0);
        q_tables(st, tails, K, g0, np_g, nint, deg, d_tab, plane, d_mass + g0, d_mean + g0);
        const int64_t pt0 = S.probs[g0].x_off;
        const int64_t npts = (g0 + np_g < B ? S.probs[g0 + np_g].x_off : S.n_tot) - pt0;
        if (npts > 0) {
            tm.begin(st);
            const dim3 grid((unsigned)((npts + Q_THREADS - 1) / Q_THREADS));           // of the one-thread-per-point kernels
            if (sample) {
                int64_t n_max = 0;
                for (int i = g0; i < g0 + np_g; ++i) n_max = std::max(n_max, S.probs[i].n);
                unsigned threads, gy;
                L.geometry(npts, n_max, threads, gy);
                hipLaunchKernelGGL(L.kernel, dim3((unsigned)np_g, gy), dim3(threads), L.lds_bytes, st, K.probs + g0,
                                   (const QDraw *)K.d_in[0] + g0, nint, K.coef, (const double *)d_tab, K.gx, K.gw, deg, smp->seed,
                                   (int)(smp->flags & MLMC_SAMPLE_ANTITHETIC), d_out, d_lower, (const double *)nullptr, (int64_t)0,
                                   (int64_t)0, (int64_t)0, (int64_t)0, sobol ? pack.at<uint64_t>(K, at_sobol) : nullptr);
            } else {
                hipLaunchKernelGGL(mode != Q_CDF ? k_q_quantile : k_q_cdf, grid, dim3(Q_THREADS), 0, st, K.probs + g0, np_g, nint, pt0, npts,
                                   K.coef, (const double *)d_tab, K.gx, K.gw, deg, d_x, d_out);
            }
            if (tails)                           // the quantiles, as k_q_quantile has just written them, are the points
                hipLaunchKernelGGL(k_q_tails, grid, dim3(Q_THREADS), 0, st, K.probs + g0, np_g, nint, pt0, npts, K.coef, (const double *)d_tab,
                                   plane, K.gx, K.gw, deg, (const double *)d_out, d_lower, d_upper);
            tm.end(st);
        }
        MLMC_HIP_CHECK(hipGetLastError());
    }
    if (stage) MLMC_HIP_CHECK(hipMemcpyAsync(out, d_out, sizeof(double) * np, hipMemcpyDeviceToHost, st));
    if (stage && lower_out) MLMC_HIP_CHECK(hipMemcpyAsync(lower_out, d_lower, sizeof(double) * np, hipMemcpyDeviceToHost, st));
    if (stage && tails) MLMC_HIP_CHECK(hipMemcpyAsync(upper_out, d_upper, sizeof(double) * np, hipMemcpyDeviceToHost, st));
    if (mass_out || mean_out) MLMC_HIP_CHECK(hipMemcpyAsync(K.h[0], d_mass, sizeof(double) * nm, hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(wait_stream(st));
    if (mass_out) std::memcpy(mass_out, K.h[0], sizeof(double) * B);
    if (mean_out) std::memcpy(mean_out, K.h[0] + B, sizeof(double) * B);
    tm.collect();
    meb_ws().trim(MEB_KEEP_BYTES);
    return 0;
}

// the sets of mlmc_density_sample_conditional_batch: y = shift[b][m] + (F z)[m] for b < B, draws and uniforms of problem m at row
// rows[m] (NULL: m) of the set's ld_rows rows
struct QSets {
    int32_t B;
    const double *shift;              // [B][M] or NULL: zeros
    const int32_t *rows;              // [M] or NULL
    int32_t ld_rows;
    const double *scale = nullptr;    // [B] or NULL: ones; read with a t copula only (mlmc_density_sample_conditional_t_batch)
};

// the Student-t copula of mlmc_density_sample_joint_t_batch: y = (F z) s with the mixing scale s[j] of draw j (copula_t.hip);
// the conditional t entry draws s with dof_mix degrees of freedom and maps with dof
struct QTCop {
    double dof;
    uint32_t mix_stream;
    double *s_out;                    // [n] or NULL
    double dof_mix;
};

// mlmc_density_sample_joint_batch (sets == NULL) and mlmc_density_sample_conditional_batch: draws of M problems joined by a
// Gaussian copula.  Table, masses and inversion are those of q_on_rule's sampling branch; the uniforms come from copula.hip
// instead of q_uniform.  The draws are processed in blocks of nb columns: latent normals Z [K][nb], copula uniforms U [M][nb],
// inversion of the block.  No value depends on nb.
// The joint entry: Z and U live in the workspace unless the caller's device arrays take them in place.
// The conditional entry: the same draws for B sets at once.  Table, masses, normals and the chain of the product are made once per
// block for all sets; the uniforms U [B][M][nb] always live in the workspace (k_cop_uniforms<true>, set on blockIdx.z), and the
// SETS instance of k_q_sample inverts them and writes draw and uniform at row rows[m] of set b.  Host arrays are staged compactly
// ([B][M][n]) and come back in runs of consecutive rows, so the rows that `rows` does not name are not touched.  No value
// depends on B.
// The joint t entry (tc != NULL, sets == NULL): the mixing scales s [nb] of the block come first (k_cop_mixing), the product stores
// y = (F z) s in U (the TSCALE instance of k_cop_uniforms) and k_tcop_map maps U in place; s lives next to Z in the workspace, beyond
// the bound that sizes the block (8 bytes per draw), unless the caller's device array takes it.
// The conditional t entry (tc != NULL, sets != NULL): blocks, workspace, staging and rows are the conditional entry's, s the joint
// t entry's with the constants of dof_mix; the SHIFT and TSCALE instance of k_cop_uniforms stores y = shift + ((F z) s) scale[b] for
// every set and k_tcop_map maps the B * M rows in place with the constants of dof.
static int q_copula(const char *fn, int32_t M, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda, const double *sigma,
                    const double *a, const double *b, int32_t n_intervals, int32_t gauss_degree, int32_t Kf, const double *factor,
                    uint64_t seed, const uint32_t *streams, int64_t first, int64_t n, int32_t flags, const QSets *sets, double *out,
                    double *u_out, double *z_out, double *mass_out, int mem_kind, const QTCop *tc = nullptr) {
    if (const int r = q_head(fn, "M", M, bases && R1 && lambda && sigma && a && b)) return r > 0;
    int nint, deg;
    if (q_rule(fn, n_intervals, gauss_degree, nint, deg, mem_kind)) return 1;
    if (q_sample_flags(fn, flags)) return 1;
    const bool sobol = flags & MLMC_SAMPLE_SOBOL;
    if (tc && tcop_check_dof(fn, tc->dof)) return 1;
    if (tc && sets && tcop_check_dof(fn, tc->dof_mix, TCOP_MAX_DOF_MIX, "dof_mix")) return 1;
    if (Kf < 1) return fail(std::string(fn) + ": K < 1");
    if (!factor) return fail(std::string(fn) + ": null factor");
    if (n < 0) return fail(std::string(fn) + ": n < 0");
    if (first < 0) return fail(std::string(fn) + ": first < 0");
    if (first > INT64_MAX - n) return fail(std::string(fn) + ": first + n overflows int64");
    if (sobol && first + n > SOBOL_MAX_INDEX) return fail(std::string(fn) + ": first + n is beyond the 2^52 points of the Sobol' sequence");
    // MLMC_SAMPLE_SOBOL: the rows of the call's distinct dimensions; latent normal k names its row instead of its stream
    std::vector<uint64_t> sobol_tab;
    std::vector<uint32_t> sobol_slot;
    if (sobol && sobol_call_table(fn, "latent normal", seed, streams, Kf, sobol_tab, sobol_slot)) return 1;
    // the mixing variable must not share its uniforms with a latent normal; under MLMC_SAMPLE_SOBOL it has a table row of its own
    std::vector<uint64_t> mix_tab;
    std::vector<uint32_t> mix_slot;
    if (tc) {
        for (int k = 0; k < Kf; ++k)
            if ((streams ? streams[k] : (uint32_t)k) == tc->mix_stream)
                return fail(std::string(fn) + ": mix_stream equals the stream of latent normal " + std::to_string(k));
        if (sobol && sobol_call_table(fn, "mixing variable", seed, &tc->mix_stream, 1, mix_tab, mix_slot)) return 1;
    }
    const int32_t B = sets ? sets->B : 1;
    const int32_t *rows = sets ? sets->rows : nullptr;
    const int32_t ld_rows = sets ? sets->ld_rows : M;
    if (sets) {
        if (B < 1) return fail(std::string(fn) + ": B < 1");
        if (ld_rows < M) return fail(std::string(fn) + ": ld_rows < M");
        for (int m = 0; rows && m < M; ++m)
            if (rows[m] < 0 || rows[m] >= ld_rows || (m > 0 && rows[m] <= rows[m - 1]))
                return fail(std::string(fn) + ": rows must be strictly increasing within 0 .. ld_rows - 1 (entry " + std::to_string(m) + ")");
        if (n > 0 && (int64_t)B * ld_rows > INT64_MAX / 8 / n) return fail(std::string(fn) + ": B * ld_rows * n overflows int64");
    }
    // a row of the factor has unit norm; under a condition it has the norm of what the condition leaves, at most 1
    for (int m = 0; m < M; ++m) {
        const double *row = factor + (size_t)m * Kf;
        double ss = 0.0;
        for (int k = 0; k < Kf; ++k) ss += row[k] * row[k];          // a value that is not finite makes the sum not finite
        if (!std::isfinite(ss)) return fail(std::string(fn) + ": factor row " + std::to_string(m) + ": an entry is not finite");
        if (sets ? !(ss <= 1.0 + 1e-6) : !(std::fabs(ss - 1.0) <= 1e-6))
            return fail(std::string(fn) + ": factor row " + std::to_string(m) +
                        (sets ? ": the sum of squares must be at most 1 + 1e-6" : ": the sum of squares must be 1 within 1e-6"));
    }
    const size_t BM = (size_t)B * (size_t)M;
    if (sets) {
        for (int64_t i = 0; sets->shift && i < (int64_t)B * M; ++i)
            if (!std::isfinite(sets->shift[i]))
                return fail(std::string(fn) + ": shift of set " + std::to_string(i / M) + ", row " + std::to_string(i % M) + " is not finite");
        for (int b = 0; tc && sets->scale && b < B; ++b)
            if (!(std::isfinite(sets->scale[b]) && sets->scale[b] > 0.0))
                return fail(std::string(fn) + ": scale of set " + std::to_string(b) + " must be finite and positive");
        if (sizeof(double) * 64 * (BM + (size_t)Kf) > Q_JOINT_BYTES)
            return fail(std::string(fn) + ": the uniforms of B * M = " + std::to_string(BM) +
                        " rows do not fit into the workspace even for a block of 64 draws; split the sets across calls (no value depends on B)");
    }
    QSetup S;
    const std::vector<int64_t> counts((size_t)M, n);
    if (q_prepare(fn, false, M, bases, R1, lambda, sigma, a, b, counts.data(), S)) return 1;
    const std::vector<QDraw> draws = q_draw_table(S);
    if (n > 0 && !out) return fail(std::string(fn) + ": null argument");
    if (n == 0 && !mass_out) return 0;
    hipStream_t st = rt().stream;
    const bool stage = mem_kind == MLMC_HOST && n > 0;
    // where a set's draws go: rows[m] of the caller's device array [B][ld_rows][n], or row m of the compact staged one [B][M][n]
    const int64_t x_set = (stage ? (int64_t)M : (int64_t)ld_rows) * n;
    if (!stage && rows)
        for (int m = 0; m < M; ++m) S.probs[m].x_off = (int64_t)rows[m] * n;
    const auto [G, plane] = q_groups(M, 1, nint);
    // the draws of a block: Z and U of a block within Q_JOINT_BYTES, whole tiles of the matrix kernel
    int64_t nb = std::max<int64_t>(64, (int64_t)(Q_JOINT_BYTES / (sizeof(double) * (BM + (size_t)Kf))) / 64 * 64);
    if (const char *env = std::getenv("MLMC_JOINT_BLOCK_DRAWS")) {
        const long long v = std::atoll(env);
        if (v > 0) nb = v;
    }
    nb = std::min(nb, std::max<int64_t>(n, 1));
    const bool z_ws = n > 0 && !(mem_kind == MLMC_DEVICE && z_out), u_ws = n > 0 && (sets || !(mem_kind == MLMC_DEVICE && u_out));
    const bool s_ws = tc && n > 0 && !(mem_kind == MLMC_DEVICE && tc->s_out);
    // what goes up with the block: the draws table | the streams (uint32) | the factor | the shifts of the sets | the Sobol' table
    // (uint64) | the mixing variable's table | the scales of the sets; a call without draws sends the draws table alone
    QPack pack;
    pack.add(draws.data(), draws.size());
    std::vector<uint32_t> sv(n > 0 ? (size_t)Kf : 0);
    for (size_t k = 0; k < sv.size(); ++k) sv[k] = sobol ? sobol_slot[k] : streams ? streams[k] : (uint32_t)k;
    const size_t at_streams = pack.add(sv.data(), sv.size()), at_factor = pack.add(factor, n > 0 ? (size_t)M * Kf : 0);
    const size_t at_shift = sets ? pack.add(sets->shift, n > 0 ? BM : 0) : 0, at_sobol = pack.add(sobol_tab.data(), n > 0 ? sobol_tab.size() : 0);
    const size_t at_mix = pack.add(mix_tab.data(), n > 0 ? mix_tab.size() : 0);
    const std::vector<double> ones(sets && tc && !sets->scale && n > 0 ? (size_t)B : 0, 1.0);
    const size_t at_scale = sets && tc ? pack.add(sets->scale ? sets->scale : ones.data(), n > 0 ? (size_t)B : 0) : 0;
    const size_t n_in = pack.data.size(), n_stage = stage ? BM * (size_t)n : 0;
    QBlock K;
    if (q_stage(S, deg, {n_in}, {(size_t)M, (size_t)plane, n_stage, u_ws ? BM * (size_t)nb : 0, z_ws ? (size_t)Kf * (size_t)nb : 0,
                                sets && u_out ? n_stage : 0, s_ws ? (size_t)nb : 0},
                {(size_t)M}, K))
        return 1;
    if (K.upload({pack.data.data()}, n_in)) return 1;
    const QDraw *d_draws = pack.at<QDraw>(K, 0);
    const uint32_t *d_streams = pack.at<uint32_t>(K, at_streams);
    const double *d_factor = pack.at<double>(K, at_factor), *d_shift = pack.at<double>(K, at_shift);
    const uint64_t *d_sobol = pack.at<uint64_t>(K, at_sobol);
    const uint64_t *d_mix = tc && sobol ? pack.at<uint64_t>(K, at_mix) : nullptr;
    const double *d_scale = pack.at<double>(K, at_scale);
    // the constants of the map and those of the mixing scale: the same but for the conditional t entry
    const TCopConst tconst = tc ? tcop_constants(tc->dof) : TCopConst{};
    const TCopConst tmix = tc && sets ? tcop_constants(tc->dof_mix) : tconst;
    double *d_mass = K.d[0], *d_tab = K.d[1], *d_out = stage ? K.d[2] : out;
    // the uniforms k_q_sample writes next to the draws: those of the sets; the joint entry's U is the output itself
    double *d_u = !sets ? nullptr : stage && u_out ? K.d[5] : u_out;
    const QSampleLaunch L = q_sample_launch(S, nint, deg, true, sets != nullptr, sobol);
    QTiming &tm = q_call_timing();
    for (int g0 = 0; g0 < M; g0 += G) {
        const int np_g = std::min(G, M - g0);
        q_tables(st, false, K, g0, np_g, nint, deg, d_tab, plane, d_mass + g0, nullptr);
        for (int64_t c0 = 0; c0 < n; c0 += nb) {
            const int64_t nc = std::min(nb, n - c0);
            // the block's Z and U: in the caller's device arrays at column c0 (row length n), or in the workspace (row length nb)
            double *Z = z_ws ? K.d[4] : z_out + c0, *U = u_ws ? K.d[3] : u_out + c0;
            const int64_t ldz = z_ws ? nb : n, ldu = u_ws ? nb : n;
            double *Sc = !tc ? nullptr : s_ws ? K.d[6] : tc->s_out + c0;
            tm.begin(st);
            if (tc && (g0 == 0 || s_ws))       // as the normals below
                cop_launch_mixing(st, tmix, seed, tc->mix_stream, d_mix, first + c0, nc, (int)(flags & MLMC_SAMPLE_ANTITHETIC), Sc);
            if ((g0 == 0 || z_ws) && sobol)    // a later group finds the normals of the block in the caller's array
                cop_launch_sobol_normals(st, d_sobol, d_streams, Kf, first + c0, nc, Z, ldz);
            else if (g0 == 0 || z_ws)
                cop_launch_normals(st, seed, d_streams, Kf, first + c0, nc, (int)(flags & MLMC_SAMPLE_ANTITHETIC), Z, ldz);
            if (sets && tc) {
                cop_launch_scaled_shifted(st, d_factor + (size_t)g0 * Kf, np_g, Kf, Z, ldz, nc, U + (int64_t)g0 * ldu, ldu, d_shift + g0, Sc,
                                          d_scale, B, M);
                // the rows of a set's group are consecutive; those of all sets are when the group is the whole set
                if (np_g == M)
                    cop_launch_t_map(st, tconst, (int)BM, nc, U, ldu);
                else
                    for (int b = 0; b < B; ++b) cop_launch_t_map(st, tconst, np_g, nc, U + ((int64_t)b * M + g0) * ldu, ldu);
            } else if (sets)
                cop_launch_uniforms_shifted(st, d_factor + (size_t)g0 * Kf, np_g, Kf, Z, ldz, nc, U + (int64_t)g0 * ldu, ldu, d_shift + g0, B, M);
            else if (tc) {
                cop_launch_scaled_product(st, d_factor + (size_t)g0 * Kf, np_g, Kf, Z, ldz, nc, U + (int64_t)g0 * ldu, ldu, Sc);
                cop_launch_t_map(st, tconst, np_g, nc, U + (int64_t)g0 * ldu, ldu);
            } else
                cop_launch_uniforms(st, d_factor + (size_t)g0 * Kf, np_g, Kf, Z, ldz, nc, U + (int64_t)g0 * ldu, ldu);
            unsigned threads, gy;
            L.geometry((int64_t)B * np_g * nc, nc, threads, gy);
            for (int b0 = 0; b0 < B; b0 += 65535)         // set of a launch = blockIdx.z; the joint entry has the one
                hipLaunchKernelGGL(L.kernel, dim3((unsigned)np_g, gy, (unsigned)std::min(B - b0, 65535)), dim3(threads), L.lds_bytes, st,
                                   K.probs + g0, d_draws + g0, nint, K.coef, (const double *)d_tab, K.gx, K.gw, deg, seed, 0,
                                   d_out + b0 * x_set + c0, d_u ? d_u + b0 * x_set + c0 : (double *)nullptr,
                                   (const double *)(U + ((int64_t)b0 * M + g0) * ldu), ldu, nc, sets ? (int64_t)M : (int64_t)0,
                                   sets ? x_set : (int64_t)0, (const uint64_t *)nullptr);
            tm.end(st);
            MLMC_HIP_CHECK(hipGetLastError());
            if (stage && z_out && g0 == 0)
                MLMC_HIP_CHECK(hipMemcpy2DAsync(z_out + c0, sizeof(double) * n, Z, sizeof(double) * ldz, sizeof(double) * nc, (size_t)Kf,
                                                hipMemcpyDeviceToHost, st));
            if (tc && stage && tc->s_out && g0 == 0)
                MLMC_HIP_CHECK(hipMemcpyAsync(tc->s_out + c0, Sc, sizeof(double) * nc, hipMemcpyDeviceToHost, st));
            if (!sets && stage && u_out)
                MLMC_HIP_CHECK(hipMemcpy2DAsync(u_out + (int64_t)g0 * n + c0, sizeof(double) * n, U + (int64_t)g0 * ldu, sizeof(double) * ldu,
                                                sizeof(double) * nc, (size_t)np_g, hipMemcpyDeviceToHost, st));
        }
        MLMC_HIP_CHECK(hipGetLastError());
    }
    if (!sets && stage) MLMC_HIP_CHECK(hipMemcpyAsync(out, d_out, sizeof(double) * (size_t)M * (size_t)n, hipMemcpyDeviceToHost, st));
    // a staged array of sets comes back in runs of consecutive rows: run m0 .. m1 - 1 of every set in one strided copy
    for (int m0 = 0, m1; sets && stage && m0 < M; m0 = m1) {
        for (m1 = m0 + 1; m1 < M && (rows ? rows[m1] == rows[m1 - 1] + 1 : true); ++m1) {}
        const int64_t to = (int64_t)(rows ? rows[m0] : m0) * n, from = (int64_t)m0 * n;
        const size_t width = sizeof(double) * (size_t)(m1 - m0) * (size_t)n, dpitch = sizeof(double) * (size_t)ld_rows * (size_t)n;
        MLMC_HIP_CHECK(hipMemcpy2DAsync(out + to, dpitch, d_out + from, sizeof(double) * (size_t)x_set, width, (size_t)B,
                                        hipMemcpyDeviceToHost, st));
        if (u_out)
            MLMC_HIP_CHECK(hipMemcpy2DAsync(u_out + to, dpitch, d_u + from, sizeof(double) * (size_t)x_set, width, (size_t)B,
                                            hipMemcpyDeviceToHost, st));
    }
    if (mass_out) MLMC_HIP_CHECK(hipMemcpyAsync(K.h[0], d_mass, sizeof(double) * M, hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(wait_stream(st));
    if (mass_out) std::memcpy(mass_out, K.h[0], sizeof(double) * M);
    tm.collect();
    meb_ws().trim(MEB_KEEP_BYTES);
    return 0;
}

// mlmc_density_scores_batch: normal scores of the stored samples of M problems, device arrays [M][ld] in place.  Table and masses
// are those of q_on_rule's CDF branch.
static int q_scores(const char *fn, int32_t M, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda, const double *sigma,
                    const double *a, const double *b, int32_t n_intervals, int32_t gauss_degree, const double *fine, const double *coarse,
                    int64_t n, int64_t ld_in, double *z_fine, double *z_coarse, int64_t ld_out, double *u_fine, double *u_coarse,
                    double *mass_out) {
    if (const int r = q_head(fn, "M", M, bases && R1 && lambda && sigma && a && b)) return r > 0;
    int nint, deg;
    if (q_rule(fn, n_intervals, gauss_degree, nint, deg)) return 1;
    if (n < 0) return fail(std::string(fn) + ": n < 0");
    if (ld_in < n || ld_out < n) return fail(std::string(fn) + ": ld_in and ld_out must be at least n");
    if (ld_in > INT64_MAX / 8 / M || ld_out > INT64_MAX / 8 / M) return fail(std::string(fn) + ": M * ld overflows int64");
    QSetup S;
    const std::vector<int64_t> counts((size_t)M, n);
    if (q_prepare(fn, false, M, bases, R1, lambda, sigma, a, b, counts.data(), S)) return 1;
    const std::vector<QDraw> draws = q_draw_table(S);
    if (!coarse) z_coarse = u_coarse = nullptr;
    if (n > 0 && (!fine || !z_fine || (coarse && !z_coarse))) return fail(std::string(fn) + ": null argument");
    if (n == 0 && !mass_out) return 0;
    if (n > 0) {
        // the bytes an array [M][ld] with n columns used spans; an output may overlap neither an input nor another output
        const auto span = [&](const double *p, int64_t ld) {
            return std::pair<uintptr_t, uintptr_t>((uintptr_t)p, (uintptr_t)p + (p ? sizeof(double) * (uintptr_t)((M - 1) * ld + n) : 0));
        };
        const std::pair<uintptr_t, uintptr_t> in[2] = {span(fine, ld_in), span(coarse, ld_in)};
        const double *outs[4] = {z_fine, z_coarse, u_fine, u_coarse};
        for (int i = 0; i < 4; ++i) {
            if (!outs[i]) continue;
            const auto o = span(outs[i], ld_out);
            for (int k = 0; k < 2; ++k)
                if ((k == 0 || coarse) && o.first < in[k].second && in[k].first < o.second)
                    return fail(std::string(fn) + ": an output array overlaps an input array");
            for (int k = 0; k < i; ++k) {
                if (!outs[k]) continue;
                const auto q = span(outs[k], ld_out);
                if (o.first < q.second && q.first < o.second) return fail(std::string(fn) + ": two output arrays overlap");
            }
        }
    }
    hipStream_t st = rt().stream;
    const auto [G, plane] = q_groups(M, 1, nint);
    const size_t n_draw = draws.size() * (sizeof(QDraw) / sizeof(double));
    QBlock K;
    if (q_stage(S, deg, {n_draw}, {(size_t)M, (size_t)plane}, {(size_t)M}, K)) return 1;
    if (K.upload({(const double *)draws.data()}, n_draw)) return 1;
    const QDraw *d_draws = (const QDraw *)K.d_in[0];
    double *d_mass = K.d[0], *d_tab = K.d[1];
    const QLdsPlan plan = q_lds_plan(S, nint, deg);
    const auto kernel = plan.row_lds ? k_q_scores<true, true> : plan.coef_lds ? k_q_scores<true, false> : k_q_scores<false, false>;
    const size_t lds_bytes = plan.bytes;
    const int64_t wg_cols = (coarse ? 1 : 2) * Q_SCORE_THREADS, launch_cols = 65535 * wg_cols;     // a grid has 65535 blocks in y
    QTiming &tm = q_call_timing();
    for (int g0 = 0; g0 < M; g0 += G) {
        const int np_g = std::min(G, M - g0);
        q_tables(st, false, K, g0, np_g, nint, deg, d_tab, plane, d_mass + g0, nullptr);
        if (n > 0) {
            tm.begin(st);
            const int64_t in_off = (int64_t)g0 * ld_in, out_off = (int64_t)g0 * ld_out;
            for (int64_t c0 = 0; c0 < n; c0 += launch_cols) {
                const unsigned gy = (unsigned)((std::min(launch_cols, n - c0) + wg_cols - 1) / wg_cols);
                hipLaunchKernelGGL(kernel, dim3((unsigned)np_g, gy), dim3(Q_SCORE_THREADS), lds_bytes, st, K.probs + g0, d_draws + g0, nint,
                                   K.coef, (const double *)d_tab, K.gx, K.gw, deg, fine + in_off, coarse ? coarse + in_off : nullptr, c0, n,
                                   ld_in, z_fine + out_off, z_coarse ? z_coarse + out_off : nullptr, ld_out,
                                   u_fine ? u_fine + out_off : nullptr, u_coarse ? u_coarse + out_off : nullptr);
            }
            tm.end(st);
        }
        MLMC_HIP_CHECK(hipGetLastError());
    }
    if (mass_out) MLMC_HIP_CHECK(hipMemcpyAsync(K.h[0], d_mass, sizeof(double) * M, hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(wait_stream(st));
    if (mass_out) std::memcpy(mass_out, K.h[0], sizeof(double) * M);
    tm.collect();
    meb_ws().trim(MEB_KEEP_BYTES);
    return 0;
}

// mlmc_density_divergences_batch
static int q_divergences(const char *fn, int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                         const double *sigma, const double *a, const double *b, int32_t n_intervals, int32_t gauss_degree, int64_t P,
                         const int32_t *first, const int32_t *second, const double *lo, const double *hi, double *out) {
    // the head in line, not q_head: P < 0 is an error of a call without problems too
    if (!rt().ready) return fail("mlmc_init has not been called (no HIP device bound)");
    if (B < 0) return fail(std::string(fn) + ": B < 0");
    if (P < 0) return fail(std::string(fn) + ": P < 0");
    if (B == 0 || P == 0) return 0;
    if (!bases || !R1 || !lambda || !sigma || !a || !b || !first || !second || !out) return fail(std::string(fn) + ": null argument");
    if (!lo != !hi) return fail(std::string(fn) + ": lo and hi must both be given or both be NULL");
    int nint, deg;
    if (q_rule(fn, n_intervals, gauss_degree, nint, deg)) return 1;
    QSetup S;
    const std::vector<int64_t> no_points(B, 0);
    if (q_prepare(fn, false, B, bases, R1, lambda, sigma, a, b, no_points.data(), S)) return 1;
    const auto pair_fail = [fn](int64_t k, const std::string &what) {
        return fail(std::string(fn) + ": pair " + std::to_string(k) + ": " + what);
    };
    std::vector<QPair> pairs((size_t)P);
    int max_coef = 0;
    for (int64_t k = 0; k < P; ++k) {
        QPair &pr = pairs[(size_t)k];
        pr.first = first[k];
        pr.second = second[k];
        if (pr.first < 0 || pr.first >= B || pr.second < 0 || pr.second >= B) return pair_fail(k, "problem index outside 0..B-1");
        const QProb &p = S.probs[pr.first], &q = S.probs[pr.second];
        const double in_lo = std::max(p.a, q.a), in_hi = std::min(p.b, q.b);
        if (!lo && !(in_lo < in_hi)) return pair_fail(k, "the two domains do not intersect");
        pr.lo = lo ? lo[k] : in_lo;
        pr.hi = lo ? hi[k] : in_hi;
        if (!(std::isfinite(pr.lo) && std::isfinite(pr.hi) && pr.lo < pr.hi)) return pair_fail(k, "the interval must be finite with lo < hi");
        if (pr.lo < in_lo || pr.hi > in_hi) return pair_fail(k, "the interval is not inside both domains");
        max_coef = std::max(max_coef, p.n_coef + q.n_coef);
    }
    const size_t lds = sizeof(double) * (size_t)max_coef;
    if (lds > 65536) return fail(std::string(fn) + ": more than 8192 terms in the two bases of a pair");
    const size_t row = (size_t)MLMC_DIV_COUNT * nint, n_out = (size_t)MLMC_DIV_COUNT * (size_t)P;
    const int64_t G = (int64_t)std::min<size_t>((size_t)P, std::max<size_t>(1, Q_TABLE_BYTES / (sizeof(double) * row)));
    hipStream_t st = rt().stream;
    QBlock K;
    if (q_stage(S, deg, {3 * (size_t)P}, {n_out, row * (size_t)G}, {n_out}, K)) return 1;
    if (K.upload({(const double *)pairs.data()}, 3 * (size_t)P)) return 1;
    const unsigned threads = (unsigned)std::min(Q_DIV_THREADS, (nint + 63) / 64 * 64);
    for (int64_t g0 = 0; g0 < P; g0 += G) {              // groups share the table, in stream order
        const int64_t np_g = std::min(G, P - g0);
        hipLaunchKernelGGL(k_q_divergences, dim3((unsigned)np_g), dim3(threads), lds, st, K.probs, (const QPair *)K.d_in[0] + g0, nint, K.coef,
                           K.gx, K.gw, deg, K.d[1], K.d[0] + g0 * MLMC_DIV_COUNT);
        MLMC_HIP_CHECK(hipGetLastError());
    }
    MLMC_HIP_CHECK(hipMemcpyAsync(K.h[0], K.d[0], sizeof(double) * n_out, hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(wait_stream(st));
    std::memcpy(out, K.h[0], sizeof(double) * n_out);
    meb_ws().trim(MEB_KEEP_BYTES);
    return 0;
}

// the LDS layout of a moments launch from the call's largest column count and coefficient count: as many whole cells per step as
// the four waves can take (at most the rule's), the columns in as few chunks as leave room for them, never fewer than one cell.
// No sum depends on it.
static QMomLayout q_mom_layout(int n_col_max, int max_coef, int nint, int deg) {
    QMomLayout L;
    L.coef_cap = max_coef;
    L.cpw = std::max(1, 64 / deg);
    const int want = std::min(4 * L.cpw, nint);
    const size_t room = Q_MOM_LDS_BYTES / sizeof(double) - (size_t)max_coef;
    const auto cells = [&](int chunk) { return (int)(room / ((size_t)deg * (chunk | 1) + chunk)); };
    L.chunk = n_col_max;
    while (cells(L.chunk) < want && L.chunk > 16) L.chunk = (L.chunk + 1) / 2;
    L.stride = L.chunk | 1;
    L.cps = std::min(want, cells(L.chunk));
    return L;
}

// mlmc_density_moments_batch
static int q_moments(const char *fn, int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                     const double *sigma, const double *a, const double *b, int32_t n_intervals, int32_t gauss_degree,
                     const mlmc_basis *const *test, const int32_t *K, double *out, double *mass_out, double *entropy_out) {
    if (const int r = q_head(fn, "B", B, bases && R1 && lambda && sigma && a && b && test && K && out)) return r > 0;
    int nint, deg;
    if (q_rule(fn, n_intervals, gauss_degree, nint, deg)) return 1;
    QSetup S;
    const std::vector<int64_t> no_points(B, 0);
    if (q_prepare(fn, false, B, bases, R1, lambda, sigma, a, b, no_points.data(), S)) return 1;
    std::vector<QTest> tests((size_t)B);
    int k_max = 0, n_col_max = 0, max_coef = 0;
    for (int i = 0; i < B; ++i) {
        const mlmc_basis *tb = test[i];
        if (!tb) return meb_fail(fn, i, "null test basis");
        if (tb->p.kind != MLMC_LEGENDRE && tb->p.kind != MLMC_MONOMIAL && tb->p.kind != MLMC_FOURIER && tb->p.kind != MLMC_SPLINE)
            return meb_fail(fn, i, "unsupported test basis kind");
        const int max_out = tb->out_size > 0 ? tb->out_size : tb->p.size;
        if (K[i] < 1 || K[i] > max_out) return meb_fail(fn, i, "K out of range");
        QTest &t = tests[(size_t)i];
        t.bp = tb->p;
        t.S = tb->out_size > 0 ? tb->p.size : K[i];
        t.reserved = 0;
        if (t.S > Q_MOM_MAX_TERMS) return meb_fail(fn, i, "more than 512 terms in the test basis");
        k_max = std::max(k_max, (int)K[i]);
        n_col_max = std::max(n_col_max, t.S + 2);
        max_coef = std::max(max_coef, S.probs[(size_t)i].n_coef);
    }
    if (max_coef > 4096) return fail(std::string(fn) + ": more than 4096 terms in the basis of a density");
    const QMomLayout L = q_mom_layout(n_col_max, max_coef, nint, deg);
    const size_t lds = sizeof(double) * ((size_t)L.coef_cap + (size_t)L.cps * ((size_t)deg * L.stride + L.chunk));
    if (L.cps < 1 || lds > Q_MOM_LDS_BYTES) return fail(std::string(fn) + ": internal error: the tile does not fit");
    const size_t n_out = (size_t)B * n_col_max, n_test = (size_t)B * (sizeof(QTest) / sizeof(double));
    hipStream_t st = rt().stream;
    QBlock Kb;
    if (q_stage(S, deg, {n_test}, {n_out}, {n_out}, Kb)) return 1;
    if (Kb.upload({(const double *)tests.data()}, n_test)) return 1;
    hipLaunchKernelGGL(k_q_moments, dim3((unsigned)B), dim3(Q_MOM_THREADS), lds, st, Kb.probs, (const QTest *)Kb.d_in[0], nint, Kb.coef, Kb.gx,
                       Kb.gw, deg, L, n_col_max, Kb.d[0]);
    MLMC_HIP_CHECK(hipGetLastError());
    MLMC_HIP_CHECK(hipMemcpyAsync(Kb.h[0], Kb.d[0], sizeof(double) * n_out, hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(wait_stream(st));
    std::vector<double> m;
    for (int i = 0; i < B; ++i) {
        const mlmc_basis *tb = test[i];
        const int terms = tests[(size_t)i].S;
        const double *row = Kb.h[0] + (size_t)i * n_col_max;
        double *o = out + (size_t)i * k_max;
        m.resize((size_t)terms);
        for (int r = 0; r < terms; ++r) m[(size_t)r] = tb->scale_c[(size_t)r] * row[r];
        for (int j = 0; j < k_max; ++j) {
            double v = 0.0;
            if (j < K[i] && tb->out_size > 0) {
                const double *mr = tb->matrix.data() + (size_t)j * tb->p.size;
                for (int r = 0; r < terms; ++r) v += mr[r] * m[(size_t)r];         // in r order, plain fp64 (no contraction in this file)
            } else if (j < K[i]) {
                v = m[(size_t)j];
            }
            o[j] = v;
        }
        if (mass_out) mass_out[i] = row[terms];
        if (entropy_out) entropy_out[i] = row[terms + 1];
    }
    meb_ws().trim(MEB_KEEP_BYTES);
    return 0;
}

}  // namespace mlmc

using namespace mlmc;

extern "C" {

int mlmc_density_eval(const mlmc_basis *b, const double *lambda, const double *sigma, int32_t R1, const double *x, int64_t n,
                      double *out, int mem_kind) {
    MLMC_API_GUARD;
    if (!b) return fail("mlmc_density_eval: null argument");
    return q_eval("mlmc_density_eval", true, 1, &b, &R1, lambda, sigma, x, &n, out, mem_kind);
}

int mlmc_density_eval_batch(int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda, const double *sigma,
                            const double *x, const int64_t *n, double *out) {
    MLMC_API_GUARD;
    return q_eval("mlmc_density_eval_batch", false, B, bases, R1, lambda, sigma, x, n, out, MLMC_HOST);
}

int mlmc_density_integrate(const mlmc_basis *b, const double *lambda, const double *sigma, int32_t R1, const double *lo,
                           const double *hi, int64_t n, int32_t degree, double *out) {
    MLMC_API_GUARD;
    if (!b) return fail("mlmc_density_integrate: null argument");
    return q_integrate("mlmc_density_integrate", true, 1, &b, &R1, lambda, sigma, lo, hi, &n, degree, out);
}

int mlmc_density_integrate_batch(int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                                 const double *sigma, const double *lo, const double *hi, const int64_t *n, int32_t degree,
                                 double *out) {
    MLMC_API_GUARD;
    return q_integrate("mlmc_density_integrate_batch", false, B, bases, R1, lambda, sigma, lo, hi, n, degree, out);
}

int mlmc_density_cdf_batch(int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda, const double *sigma,
                           const double *a, const double *b, int32_t n_intervals, int32_t gauss_degree, const double *x,
                           const int64_t *n, double *out, double *mass_out, int mem_kind) {
    MLMC_API_GUARD;
    return q_on_rule("mlmc_density_cdf_batch", Q_CDF, B, bases, R1, lambda, sigma, a, b, n_intervals, gauss_degree, x, n, out, mass_out,
                     mem_kind);
}

int mlmc_density_quantiles_batch(int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                                 const double *sigma, const double *a, const double *b, int32_t n_intervals, int32_t gauss_degree,
                                 const double *p, const int64_t *n, double *out, double *mass_out, int mem_kind) {
    MLMC_API_GUARD;
    return q_on_rule("mlmc_density_quantiles_batch", Q_QUANTILES, B, bases, R1, lambda, sigma, a, b, n_intervals, gauss_degree, p, n, out,
                     mass_out, mem_kind);
}

int mlmc_density_tail_means_batch(int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                                  const double *sigma, const double *a, const double *b, int32_t n_intervals, int32_t gauss_degree,
                                  const double *p, const int64_t *n, double *q_out, double *lower_out, double *upper_out, double *mass_out,
                                  double *mean_out, int mem_kind) {
    MLMC_API_GUARD;
    return q_on_rule("mlmc_density_tail_means_batch", Q_TAILS, B, bases, R1, lambda, sigma, a, b, n_intervals, gauss_degree, p, n, q_out,
                     mass_out, mem_kind, lower_out, upper_out, mean_out);
}

int mlmc_density_sample_batch(int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda, const double *sigma,
                              const double *a, const double *b, int32_t n_intervals, int32_t gauss_degree, uint64_t seed,
                              const uint32_t *streams, const int64_t *first, const int64_t *n, int32_t flags, double *out, double *u_out,
                              double *mass_out, int mem_kind) {
    MLMC_API_GUARD;
    const QSampling smp = {seed, streams, first, flags, u_out};
    return q_on_rule("mlmc_density_sample_batch", Q_SAMPLE, B, bases, R1, lambda, sigma, a, b, n_intervals, gauss_degree, nullptr, n, out,
                     mass_out, mem_kind, nullptr, nullptr, nullptr, &smp);
}

int mlmc_density_sample_joint_batch(int32_t M, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                                    const double *sigma, const double *a, const double *b, int32_t n_intervals, int32_t gauss_degree,
                                    int32_t K, const double *factor, uint64_t seed, const uint32_t *streams, int64_t first, int64_t n,
                                    int32_t flags, double *out, double *u_out, double *z_out, double *mass_out, int mem_kind) {
    MLMC_API_GUARD;
    return q_copula("mlmc_density_sample_joint_batch", M, bases, R1, lambda, sigma, a, b, n_intervals, gauss_degree, K, factor, seed,
                    streams, first, n, flags, nullptr, out, u_out, z_out, mass_out, mem_kind);
}

int mlmc_density_sample_joint_t_batch(int32_t M, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                                      const double *sigma, const double *a, const double *b, int32_t n_intervals, int32_t gauss_degree,
                                      int32_t K, const double *factor, double dof, uint64_t seed, const uint32_t *streams,
                                      uint32_t mix_stream, int64_t first, int64_t n, int32_t flags, double *out, double *u_out,
                                      double *z_out, double *s_out, double *mass_out, int mem_kind) {
    MLMC_API_GUARD;
    const QTCop tc{dof, mix_stream, s_out, dof};
    return q_copula("mlmc_density_sample_joint_t_batch", M, bases, R1, lambda, sigma, a, b, n_intervals, gauss_degree, K, factor, seed,
                    streams, first, n, flags, nullptr, out, u_out, z_out, mass_out, mem_kind, &tc);
}

int mlmc_density_sample_conditional_batch(int32_t M, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                                          const double *sigma, const double *a, const double *b, int32_t n_intervals,
                                          int32_t gauss_degree, int32_t K, const double *factor, uint64_t seed, const uint32_t *streams,
                                          int64_t first, int64_t n, int32_t flags, int32_t B, const double *shift, const int32_t *rows,
                                          int32_t ld_rows, double *out, double *u_out, double *z_out, double *mass_out, int mem_kind) {
    MLMC_API_GUARD;
    const QSets sets = {B, shift, rows, ld_rows};
    return q_copula("mlmc_density_sample_conditional_batch", M, bases, R1, lambda, sigma, a, b, n_intervals, gauss_degree, K, factor, seed,
                    streams, first, n, flags, &sets, out, u_out, z_out, mass_out, mem_kind);
}

int mlmc_density_sample_conditional_t_batch(int32_t M, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                                            const double *sigma, const double *a, const double *b, int32_t n_intervals,
                                            int32_t gauss_degree, int32_t K, const double *factor, double dof, double dof_mix,
                                            uint64_t seed, const uint32_t *streams, uint32_t mix_stream, int64_t first, int64_t n,
                                            int32_t flags, int32_t B, const double *shift, const double *scale, const int32_t *rows,
                                            int32_t ld_rows, double *out, double *u_out, double *z_out, double *s_out, double *mass_out,
                                            int mem_kind) {
    MLMC_API_GUARD;
    const QSets sets = {B, shift, rows, ld_rows, scale};
    const QTCop tc{dof, mix_stream, s_out, dof_mix};
    return q_copula("mlmc_density_sample_conditional_t_batch", M, bases, R1, lambda, sigma, a, b, n_intervals, gauss_degree, K, factor,
                    seed, streams, first, n, flags, &sets, out, u_out, z_out, mass_out, mem_kind, &tc);
}

int mlmc_density_scores_batch(int32_t M, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda, const double *sigma,
                              const double *a, const double *b, int32_t n_intervals, int32_t gauss_degree, const double *fine,
                              const double *coarse, int64_t n, int64_t ld_in, double *z_fine, double *z_coarse, int64_t ld_out,
                              double *u_fine, double *u_coarse, double *mass_out) {
    MLMC_API_GUARD;
    return q_scores("mlmc_density_scores_batch", M, bases, R1, lambda, sigma, a, b, n_intervals, gauss_degree, fine, coarse, n, ld_in,
                    z_fine, z_coarse, ld_out, u_fine, u_coarse, mass_out);
}

int mlmc_density_divergences_batch(int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda,
                                   const double *sigma, const double *a, const double *b, int32_t n_intervals, int32_t gauss_degree,
                                   int64_t P, const int32_t *first, const int32_t *second, const double *lo, const double *hi,
                                   double *out) {
    MLMC_API_GUARD;
    return q_divergences("mlmc_density_divergences_batch", B, bases, R1, lambda, sigma, a, b, n_intervals, gauss_degree, P, first, second,
                         lo, hi, out);
}

int mlmc_density_moments_batch(int32_t B, const mlmc_basis *const *bases, const int32_t *R1, const double *lambda, const double *sigma,
                               const double *a, const double *b, int32_t n_intervals, int32_t gauss_degree,
                               const mlmc_basis *const *test, const int32_t *K, double *out, double *mass_out, double *entropy_out) {
    MLMC_API_GUARD;
    return q_moments("mlmc_density_moments_batch", B, bases, R1, lambda, sigma, a, b, n_intervals, gauss_degree, test, K, out, mass_out,
                     entropy_out);
}

int mlmc_density_quantiles_kernel_time(double *ms, int64_t *launches) {
    MLMC_API_GUARD;
    QTiming &tm = q_timing();
    if (ms) *ms = tm.ms;
    if (launches) *launches = tm.launches;
    tm.ms = 0.0;
    tm.launches = 0;
    return 0;
}

}  // extern "C"
