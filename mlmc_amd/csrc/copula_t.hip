// The Student-t copula of mlmc_density_sample_joint_t_batch on the device (gfx950), and the elementwise entries that define its
// functions (include/mlmc_hip.h): mlmc_student_t_cdf, mlmc_student_t_quantile, mlmc_chi2_mixing_scale.  The host path of the
// sampling entry is density.hip's (q_copula); the product y = (F z) (x) s is the TSCALE instance of k_cop_uniforms (copula.hip).
// mlmc_density_sample_conditional_t_batch uses the same kernels: the mixing scale with the constants of nu_c = nu + p (up to 192,
// mlmc_chi2_conditional_scale), the map with those of nu, over the rows of all sets.
//
//   k_cop_mixing : s[c] = chi2_mixing_scale(nu, p0) of draw first + c, p0 the Philox uniform of the mixing stream or the Sobol'
//                  coordinate of the mixing dimension (sobol.hpp); one thread per draw
//   k_box_mixing : the same scale for the t box entries (box_prob.hip): s[r][c] of point j0 + c under seed r, for all seeds of a
//                  call and the whole blocks of one launch; one thread per (seed, point), once per point and not once per box
//   k_box_lead_weights, k_box_lead : the conditioned lead component of the tl box entries: the lead's weight W0
//                  per box from two t CDFs, and per (seed, box, point) the lead score v by student_t_quantile inside the lead's
//                  limits and the scale sc = g0 sqrt((nu + v v) / (nu + 1)), g0 the scale k_box_mixing made with nu + 1
//   k_tcop_map   : U = clamp(student_t_cdf(nu, U)) in place, one thread per element.  The map is a kernel of its own and not the
//                  epilogue of the product: a lane of the product holds 16 accumulators, and the series loop over them would keep
//                  them and the constants of pow / exp / log1p live together (the comment at the top of copula.hip).
//   k_tcop_scores : Y = student_t_quantile(clamp(U)), NaN for NaN, one thread per element: the t scores of
//                  mlmc_copula_log_density (copula_lik.hip), a pass of its own ahead of the chain for the reason above
//   k_t_elementwise : the elementwise entries, one thread per element
//
// student_t_cdf.  With t = |y|, a = nu / 2, A = (nu + 1) / 2 and c = Gamma(A) / (sqrt(nu pi) Gamma(a)) (the density at 0, from the
// host), three regions:
//   centre, t < min(1.2, sqrt(nu)):  q = t^2 / nu, w = q / (1 + q),
//       T(-t) = 1/2 - t c (1 + q)^-A  sum_n (A)_n / (3/2)_n w^n          (Pfaff form of 2F1(1/2, A; 3/2; -q); positive terms)
//     T(-t) > 0.11 there, so the subtraction costs at most a factor 4.5 in relative accuracy; w <= 1/2 and w (nu + 1) / 3 < 1/2.
//   middle, t < sqrt(nu):  q, w as above, x = 1 / (1 + q) > 1/2,
//       T(-t) = (c / sqrt(nu)) (1 + q)^-a sqrt(w) h(x),   h the continued fraction of I_x(a, 1/2) (modified Lentz)
//     the tail series would need log(2^-56) / log(x) terms here; the fraction needs O(sqrt(nu)) steps.
//   tail:  r = sqrt(nu) / t <= 1, q = r^2, x = q / (1 + q) <= 1/2,
//       T(-t) = (c / sqrt(nu)) r^nu (1 + q)^-A  sum_n (A)_n / (a + 1)_n x^n          (I_x(a, 1/2) / 2; positive terms)
//   The powers are exp(-A log1p(q)) with q <= 1 and pow(r, nu): neither forms nu times a large logarithm, so the relative error
//   does not grow with the depth of the tail.  tests/t_copula_cases.py counts the trips: at most 55 of the series, 46 of the fraction.
// chi2_mixing_scale.  a = nu / 2, x = g / 2 solves P(a, x) = p.  P is the series x^a e^-x / Gamma(a + 1) sum_n x^n / (a + 1)_n for
//   x < a + 1, Q = 1 - P the Lentz continued fraction beyond.  Start: Wilson-Hilferty, or (p Gamma(a + 1))^(1/a) where that is small.
//   p <= 1/2: Newton on log P - log p in log x; p > 1/2: Newton on log Q - log(1 - p) in x (both nearly linear in their tail), the
//   step clamped, at most C_NEWTON_CAP steps, stop once a step is below 2^-30 relative.
// student_t_quantile.  For 0 < p <= 1/2 the root t >= 0 of t_lower(t) = p, y = -t; for p > 1/2 it is -Q(1 - p) (1 - p is exact
//   there), so that Q(1 - p) == -Q(p) bit for bit.  Start: the leading term of the tail, t = sqrt(nu) / r with
//   r = (p sqrt(nu) / c)^(1 / nu), where r < e^-0.7; else the Cornish-Fisher expansion about the normal quantile.  Halley steps on
//   g = log T(-t) - log p (near the root from the difference T - p, which is then exact), both derivatives from the closed-form
//   density f: g' = -f / T (beyond sqrt(nu) from the prefactor of the tail series: f may underflow where T does not) and
//   f' / f = -(nu + 1) t / (nu + t^2).  From the tail start the variable is log t (g is nearly linear in it there: slope -nu),
//   else t; the Halley factor is clamped to [1/2, 2] and the step to [-3, 3] (log t) or [-t / 2, max(1, t)]; at most
//   T_NEWTON_CAP steps; stop once a step is below 2^-30 of t (log t) or of max(t, T / f) (t: near p = 1/2 the root tends to 0
//   and T / f is what one rounding of p moves it by).  A lane that does not converge returns its last iterate.
//   tests/copula_lik_cases.py counts the trips: at most 3.
// Every loop has a fixed trip count.
#include <algorithm>
#include <cmath>
#include <string>

#include "copula.hpp"
#include "sobol.hpp"

namespace mlmc {

constexpr int TC_THREADS = 256;
constexpr int T_SERIES_CAP = 200;
constexpr int T_LENTZ_CAP = 200;
constexpr int C_SERIES_CAP = 400;
constexpr int C_LENTZ_CAP = 400;
constexpr int C_NEWTON_CAP = 40;
constexpr int T_NEWTON_CAP = 40;
constexpr double T_LOG_START = -0.7;                  // log r of the tail start below which the steps run in log t

TCopConst tcop_constants(double dof) {
    TCopConst c;
    c.dof = dof;
    c.sqrt_dof = std::sqrt(dof);
    c.A = 0.5 * (dof + 1.0);
    // in long double: the difference of the two log-gammas would otherwise cost every value of the call tens of ulps
    const long double nu = dof;
    c.c0 = (double)(std::exp(std::lgamma(0.5L * (nu + 1.0L)) - std::lgamma(0.5L * nu)) / std::sqrt(nu * 3.14159265358979323846264338328L));
    c.t_split = std::min(1.2, c.sqrt_dof);
    c.a = 0.5 * dof;
    c.lg_a1 = (double)std::lgamma(0.5L * nu + 1.0L);
    return c;
}

// sum_n prod_{i < n} z (A + i) / (B + i), 0 <= z < 1: positive terms; stops when a term is below 2^-56 of the sum
__device__ __forceinline__ double t_series(double A, double B, double z) {
    double term = 1.0, sum = 1.0;
    for (int n = 0; n < T_SERIES_CAP; ++n) {
        term *= z * ((A + n) / (B + n));
        sum += term;
        if (term <= sum * 0x1p-56) break;
    }
    return sum;
}

// the continued fraction of I_x(a, 1/2) (modified Lentz) in the place of the tail series, 1/2 < x < 1
__device__ __forceinline__ double t_fraction(double a, double x) {
    constexpr double tiny = 0x1p-1000;
    const double qab = a + 0.5, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= T_LENTZ_CAP; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (0.5 - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) <= 0x1p-50) break;
    }
    return h;
}

// T_nu(-t), t >= 0
__device__ double t_lower(const TCopConst &C, double t) {
    if (t < C.t_split) {
        const double q = t * t / C.dof, w = q / (1.0 + q);
        const double pre = t * C.c0 * exp(-C.A * log1p(q));
        return 0.5 - pre * t_series(C.A, 1.5, w);
    }
    if (t == __builtin_inf()) return 0.0;
    if (t < C.sqrt_dof) {
        const double q = t * t / C.dof, w = q / (1.0 + q);
        const double pre = (C.c0 / C.sqrt_dof) * exp(-C.a * log1p(q)) * sqrt(w);
        return pre * t_fraction(C.a, 1.0 / (1.0 + q));
    }
    const double r = C.sqrt_dof / t, q = r * r;
    const double pre = (C.c0 / C.sqrt_dof) * pow(r, C.dof) * exp(-C.A * log1p(q));
    return pre * t_series(C.A, C.a + 1.0, q / (1.0 + q));
}

__device__ double student_t_cdf(const TCopConst &C, double y) {
    if (y != y) return y;
    return y <= 0.0 ? t_lower(C, -y) : 1.0 - t_lower(C, y);
}

// t >= 0 with T_nu(-t) = p, 0 < p <= 1/2
__device__ double t_lower_root(const TCopConst &C, double p) {
    const double nu = C.dof;
    const double lr = log(p * C.sqrt_dof / C.c0) / nu;
    const bool in_log = lr < T_LOG_START;
    double t;
    if (in_log) {
        t = C.sqrt_dof * exp(-lr);
        if (t == __builtin_inf()) return t;            // the root is beyond the largest number
    } else {
        const double z = -normcdfinv(p), z2 = z * z;
        t = z + z * (z2 + 1.0) / (4.0 * nu) + z * ((5.0 * z2 + 16.0) * z2 + 3.0) / (96.0 * nu * nu);
    }
    for (int it = 0; it < T_NEWTON_CAP; ++it) {
        const double T = t_lower(C, t);
        double step;
        if (!(T > 0.0)) {                              // beyond where T underflows: back towards the centre
            step = in_log ? -3.0 : -0.5 * t;
        } else {
            const double rel = (T - p) / p;
            const double g = fabs(rel) < 0.5 ? log1p(rel) : log(T / p);
            // h = f / T = -g': beyond sqrt(nu) from the prefactor of the tail series, f = pre nu / t (f itself may underflow
            // where T does not); w = -f' / f
            double h;
            if (t < C.sqrt_dof)
                h = C.c0 * exp(-C.A * log1p(t * t / nu)) / T;
            else {
                const double r = C.sqrt_dof / t;
                h = (C.c0 / C.sqrt_dof) * pow(r, nu) * exp(-C.A * log1p(r * r)) / T * (nu / t);
            }
            const double w = 2.0 * C.A / (nu / t + t);
            if (in_log) {
                const double th = t * h;
                const double den = fmin(fmax(1.0 - 0.5 * g * (w / h - 1.0 - 1.0 / th), 0.5), 2.0);
                step = fmin(fmax(g / th / den, -3.0), 3.0);
            } else {
                const double den = fmin(fmax(1.0 - 0.5 * g * (w / h - 1.0), 0.5), 2.0);
                step = fmin(fmax(g / h / den, -0.5 * t), fmax(1.0, t));
                if (fabs(step) <= 0x1p-30 * fmax(t, 1.0 / h)) {
                    t += step;
                    break;
                }
            }
        }
        if (in_log) {
            t *= exp(step);
            if (fabs(step) <= 0x1p-30) break;
        } else
            t += step;
    }
    return t;
}

__device__ double student_t_quantile(const TCopConst &C, double p) {
    if (!(p >= 0.0 && p <= 1.0)) return __builtin_nan("");
    if (p == 0.0) return -__builtin_inf();
    if (p == 1.0) return __builtin_inf();
    if (p == 0.5) return 0.0;
    return p <= 0.5 ? -t_lower_root(C, p) : t_lower_root(C, 1.0 - p);
}

// P(a, x) (x < a + 1: the series) or Q(a, x) (the continued fraction), and D = x^a e^-x / Gamma(a + 1)
struct GammaPQ {
    double P, Q, D;
};
__device__ __forceinline__ GammaPQ c_gamma_pq(const TCopConst &C, double x) {
    const double a = C.a;
    double P, Q;
    const double D = exp(a * log(x) - x - C.lg_a1);
    if (x < a + 1.0) {
        double term = 1.0, sum = 1.0;
        for (int n = 0; n < C_SERIES_CAP; ++n) {
            term *= x / (a + 1.0 + n);
            sum += term;
            if (term <= sum * 0x1p-56) break;
        }
        P = D * sum;
        Q = 1.0 - P;
    } else {
        constexpr double tiny = 0x1p-1000;
        double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
        for (int i = 1; i <= C_LENTZ_CAP; ++i) {
            const double an = -(double)i * ((double)i - a);
            b += 2.0;
            d = an * d + b;
            if (fabs(d) < tiny) d = tiny;
            c = b + an / c;
            if (fabs(c) < tiny) c = tiny;
            d = 1.0 / d;
            const double del = d * c;
            h *= del;
            if (fabs(del - 1.0) <= 0x1p-50) break;
        }
        Q = a * D * h;
        P = 1.0 - Q;
    }
    return GammaPQ{P, Q, D};
}

__device__ double chi2_mixing_scale(const TCopConst &C, double p) {
    if (!(p > 0.0 && p < 1.0)) return __builtin_nan("");
    const double a = C.a;
    const bool lower = p <= 0.5;
    const double target = lower ? p : 1.0 - p;
    const double c9 = 1.0 / (9.0 * a), wh = 1.0 - c9 + normcdfinv(p) * sqrt(c9);
    const double x_small = exp((log(p) + C.lg_a1) / a);
    double x = a * wh * wh * wh;
    if (!(wh > 0.0) || x_small < 0.2 * (a + 1.0)) x = x_small;
    for (int it = 0; it < C_NEWTON_CAP; ++it) {
        const GammaPQ g = c_gamma_pq(C, x);
        const double P = g.P, Q = g.Q, D = g.D;
        const double v = lower ? P : Q;
        // log(v / target): near the root from the difference, which is then exact
        const double rel = (v - target) / target;
        const double h = fabs(rel) < 0.5 ? log1p(rel) : log(v / target);
        double step;                                    // relative: x <- x (1 + step) or x exp(step)
        if (lower) {
            step = fmin(fmax(-h * P / (a * D), -3.0), 3.0);
            x *= exp(step);
        } else {
            step = fmin(fmax(h * Q / (a * D), -0.5), 1.0);          // (x f = a D): dx / x
            x += x * step;
        }
        if (fabs(step) <= 0x1p-30) break;
    }
    return sqrt(a / x);
}

__global__ __launch_bounds__(TC_THREADS) void k_cop_mixing(TCopConst C, uint64_t seed, uint32_t stream, const uint64_t *__restrict__ sobol_row,
                                                           int64_t first, int64_t ncols, int antithetic, double *__restrict__ s) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncols) return;
    const uint64_t j = (uint64_t)(first + c);
    const double p0 = sobol_row ? sobol_unit(sobol_point(sobol_row, j)) : q_uniform(seed, stream, antithetic ? j >> 1 : j);
    s[c] = chi2_mixing_scale(C, p0);
}

// The mixing scales of the blocks of one launch of the t box entries (box_prob.hip), for every seed of the call: column c is point
// j0 + c, blockIdx.y the seed.  p0 is the Philox uniform j of `stream` under seeds[r], or with `table` the coordinate of point j in
// row `stream` of seed r's table (table_rows rows per seed).  Points outside [first, first + n) pad their block with s = 1.
__global__ __launch_bounds__(TC_THREADS) void k_box_mixing(TCopConst C, const uint64_t *__restrict__ seeds, uint32_t stream,
                                                           const uint64_t *__restrict__ table, int table_rows, int64_t j0, int64_t ncols,
                                                           int64_t first, int64_t n, double *__restrict__ s) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncols) return;
    const int r = blockIdx.y;
    const int64_t j = j0 + c;
    double v = 1.0;
    if (j >= first && j < first + n) {
        const double p0 = table ? sobol_unit(sobol_point(table + ((int64_t)r * table_rows + stream) * SOBOL_ROW, (uint64_t)j))
                                : q_uniform(seeds[r], stream, (uint64_t)j);
        v = chi2_mixing_scale(C, p0);
    }
    s[(int64_t)r * ncols + c] = v;
}

// The lead component of the tl box entries (box_prob.hip).  With a = lo[b][0] / L_00 and bq = hi[b][0] / L_00 the
// lead score V = Y_0 / L_00 is Student-t with nu degrees of freedom: w[b] = W0 = T(bq) - T(a) through the lower tail on either
// side, w[B + b] = d, the lower end of the interval of p.  One thread per box, once per call.  L_00 of box b is L[b * fstride]
// (fstride = 0: one factor for all boxes).
__global__ __launch_bounds__(TC_THREADS) void k_box_lead_weights(TCopConst C, int M, const double *__restrict__ L, int64_t fstride,
                                                                 const double *__restrict__ lo, const double *__restrict__ hi, int B,
                                                                 double *__restrict__ w) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double l00 = L[(int64_t)b * fstride], a = lo[(int64_t)b * M] / l00, bq = hi[(int64_t)b * M] / l00;
    const bool refl = a > 0.0;
    const double d = student_t_cdf(C, refl ? -bq : a), e = student_t_cdf(C, refl ? -a : bq);
    w[b] = a < bq ? e - d : 0.0;
    w[B + b] = d;
}

// v and sc of the tl box entries for the blocks of one launch: column c is point j0 + c, blockIdx.y the pair (seed r, box b) behind
// pair0.  g0 [R][ncols] are the scales k_box_mixing made with the constants of nu + 1; C holds those of nu.  The uniform of the
// lead is the Philox uniform j of `stream` under seeds[r] or the coordinate of point j in row `stream` of seed r's table.
//   p = min(max(d + w W0, 2^-1022), 1 - 2^-53), v = T^-1(p) (negated for an upper-tail lead), clamped to [a, bq] and to +-2^500;
//   sc = g0 sqrt((nu + v v) / (nu + 1)).
// W0, d, a and bq are uniform over a wave (scalar loads); v and sc are not.  Points outside [first, first + n) pad with v = 0, sc = 1.
__global__ __launch_bounds__(TC_THREADS) void k_box_lead(TCopConst C, int M, const double *__restrict__ L, int64_t fstride,
                                                         const double *__restrict__ lo, const double *__restrict__ hi, int B, int64_t pair0,
                                                         const uint64_t *__restrict__ seeds, uint32_t stream,
                                                         const uint64_t *__restrict__ table, int table_rows, int64_t j0, int64_t ncols,
                                                         int64_t first, int64_t n, const double *__restrict__ g0,
                                                         const double *__restrict__ w, double *__restrict__ v_out,
                                                         double *__restrict__ sc_out) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncols) return;
    const int64_t pair = pair0 + blockIdx.y;
    const int r = (int)(pair / B), b = (int)(pair % B);
    const int64_t j = j0 + c;
    double v = 0.0, sc = 1.0;
    if (j >= first && j < first + n) {
        const double l00 = L[(int64_t)b * fstride], a = lo[(int64_t)b * M] / l00, bq = hi[(int64_t)b * M] / l00;
        const bool refl = a > 0.0;
        const double u = table ? sobol_unit(sobol_point(table + ((int64_t)r * table_rows + stream) * SOBOL_ROW, (uint64_t)j))
                               : q_uniform(seeds[r], stream, (uint64_t)j);
        const double p = fmin(fmax(__dadd_rn(w[B + b], __dmul_rn(u, w[b])), 0x1p-1022), 1.0 - 0x1p-53);
        v = student_t_quantile(C, p);
        v = refl ? -v : v;
        v = fmin(fmax(v, a), bq);
        v = fmin(fmax(v, -0x1p500), 0x1p500);          // v v stays finite
        const double q = __dsqrt_rn(__dadd_rn(C.dof, __dmul_rn(v, v)) / __dadd_rn(C.dof, 1.0));
        sc = __dmul_rn(g0[(int64_t)r * ncols + c], q);
    }
    v_out[pair * ncols + c] = v;
    sc_out[pair * ncols + c] = sc;
}

__global__ __launch_bounds__(TC_THREADS) void k_tcop_map(TCopConst C, int64_t ncols, double *__restrict__ U, int64_t ldu) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncols) return;
    double *u = U + (int64_t)blockIdx.y * ldu + c;
    *u = fmin(fmax(student_t_cdf(C, *u), 0x1p-53), 1.0 - 0x1p-53);
}

enum { T_CDF = 0, T_CHI2 = 1, T_QUANTILE = 2 };         // the functions of k_t_elementwise

template <int FN>
__global__ __launch_bounds__(TC_THREADS) void k_t_elementwise(TCopConst C, int64_t n, const double *__restrict__ in, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = FN == T_CHI2 ? chi2_mixing_scale(C, in[i]) : FN == T_QUANTILE ? student_t_quantile(C, in[i]) : student_t_cdf(C, in[i]);
}

// Y = student_t_quantile(clamp(U)), NaN for NaN: one thread per element, blockIdx.y the row
__global__ __launch_bounds__(TC_THREADS) void k_tcop_scores(TCopConst C, int64_t ncols, const double *__restrict__ U, int64_t ldu,
                                                            double *__restrict__ Y, int64_t ldy) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncols) return;
    const double u = U[(int64_t)blockIdx.y * ldu + c];
    Y[(int64_t)blockIdx.y * ldy + c] = u != u ? u : student_t_quantile(C, fmin(fmax(u, 0x1p-53), 1.0 - 0x1p-53));
}

void cop_launch_mixing(hipStream_t st, const TCopConst &C, uint64_t seed, uint32_t stream, const uint64_t *sobol_row, int64_t first,
                       int64_t ncols, int antithetic, double *s) {
    hipLaunchKernelGGL(k_cop_mixing, dim3((unsigned)((ncols + TC_THREADS - 1) / TC_THREADS)), dim3(TC_THREADS), 0, st, C, seed, stream,
                       sobol_row, first, ncols, antithetic, s);
}

void cop_launch_box_mixing(hipStream_t st, const TCopConst &C, int R, const uint64_t *seeds, uint32_t stream, const uint64_t *table,
                           int table_rows, int64_t j0, int64_t ncols, int64_t first, int64_t n, double *s) {
    // seed of a launch = blockIdx.y: more seeds than a grid has in y go in several launches
    for (int r0 = 0; r0 < R; r0 += 65535)
        hipLaunchKernelGGL(k_box_mixing, dim3((unsigned)((ncols + TC_THREADS - 1) / TC_THREADS), (unsigned)std::min(R - r0, 65535)),
                           dim3(TC_THREADS), 0, st, C, seeds + r0, stream,
                           table ? table + (int64_t)r0 * table_rows * SOBOL_ROW : nullptr, table_rows, j0, ncols, first, n,
                           s + (int64_t)r0 * ncols);
}

void cop_launch_box_lead_weights(hipStream_t st, const TCopConst &C, int M, const double *L, int64_t fstride, const double *lo,
                                 const double *hi, int B, double *w) {
    hipLaunchKernelGGL(k_box_lead_weights, dim3((unsigned)((B + TC_THREADS - 1) / TC_THREADS)), dim3(TC_THREADS), 0, st, C, M, L, fstride, lo, hi, B, w);
}

void cop_launch_box_lead(hipStream_t st, const TCopConst &C, int M, const double *L, int64_t fstride, const double *lo, const double *hi,
                         int B, int R, const uint64_t *seeds, uint32_t stream, const uint64_t *table, int table_rows, int64_t j0, int64_t ncols,
                         int64_t first, int64_t n, const double *g0, const double *w, double *v, double *sc) {
    // pair of a launch = blockIdx.y: more pairs than a grid has in y go in several launches
    const int64_t pairs = (int64_t)R * B;
    for (int64_t p0 = 0; p0 < pairs; p0 += 65535)
        hipLaunchKernelGGL(k_box_lead, dim3((unsigned)((ncols + TC_THREADS - 1) / TC_THREADS), (unsigned)std::min<int64_t>(pairs - p0, 65535)),
                           dim3(TC_THREADS), 0, st, C, M, L, fstride, lo, hi, B, p0, seeds, stream, table, table_rows, j0, ncols, first, n, g0, w, v,
                           sc);
}

void cop_launch_t_map(hipStream_t st, const TCopConst &C, int M, int64_t ncols, double *U, int64_t ldu) {
    // row of a launch = blockIdx.y: more rows than a grid has in y go in several launches
    for (int m0 = 0; m0 < M; m0 += 65535)
        hipLaunchKernelGGL(k_tcop_map, dim3((unsigned)((ncols + TC_THREADS - 1) / TC_THREADS), (unsigned)std::min(M - m0, 65535)),
                           dim3(TC_THREADS), 0, st, C, ncols, U + (int64_t)m0 * ldu, ldu);
}

void cop_launch_t_scores(hipStream_t st, const TCopConst &C, int M, int64_t ncols, const double *U, int64_t ldu, double *Y, int64_t ldy) {
    for (int m0 = 0; m0 < M; m0 += 65535)
        hipLaunchKernelGGL(k_tcop_scores, dim3((unsigned)((ncols + TC_THREADS - 1) / TC_THREADS), (unsigned)std::min(M - m0, 65535)),
                           dim3(TC_THREADS), 0, st, C, ncols, U + (int64_t)m0 * ldu, ldu, Y + (int64_t)m0 * ldy, ldy);
}

int tcop_check_dof(const char *fn, double dof, int max_dof, const char *name) {
    if (!(dof >= 1.0 && dof <= (double)max_dof))
        return fail(std::string(fn) + ": " + name + " must lie in [1, " + std::to_string(max_dof) + "]");
    return 0;
}

static MultiWorkspace &t_ws() {
    static MultiWorkspace ws;
    return ws;
}

static int t_elementwise(const char *fn, int which, double dof, int64_t n, const double *in, double *out, int mem_kind,
                         int max_dof = TCOP_MAX_DOF, const char *dof_name = "dof") {
    if (!rt().ready) return fail("mlmc_init has not been called (no HIP device bound)");
    if (tcop_check_dof(fn, dof, max_dof, dof_name)) return 1;
    if (n < 0) return fail(std::string(fn) + ": n < 0");
    if (mem_kind != MLMC_HOST && mem_kind != MLMC_DEVICE) return fail(std::string(fn) + ": bad mem_kind");
    if (!in || !out) return fail(std::string(fn) + ": null argument");
    if (n == 0) return 0;
    hipStream_t st = rt().stream;
    const TCopConst C = tcop_constants(dof);
    const double *d_in = in;
    double *d_out = out;
    if (mem_kind == MLMC_HOST) {
        if (t_ws().reserve(2 * sizeof(double) * (size_t)n)) return 1;
        double *buf = (double *)t_ws().dev;
        MLMC_HIP_CHECK(hipMemcpyAsync(buf, in, sizeof(double) * n, hipMemcpyHostToDevice, st));
        d_in = buf;
        d_out = buf + n;
    }
    const dim3 grid((unsigned)((n + TC_THREADS - 1) / TC_THREADS));
    if (which == T_CHI2)
        hipLaunchKernelGGL(k_t_elementwise<T_CHI2>, grid, dim3(TC_THREADS), 0, st, C, n, d_in, d_out);
    else if (which == T_QUANTILE)
        hipLaunchKernelGGL(k_t_elementwise<T_QUANTILE>, grid, dim3(TC_THREADS), 0, st, C, n, d_in, d_out);
    else
        hipLaunchKernelGGL(k_t_elementwise<T_CDF>, grid, dim3(TC_THREADS), 0, st, C, n, d_in, d_out);
    MLMC_HIP_CHECK(hipGetLastError());
    if (mem_kind == MLMC_HOST) MLMC_HIP_CHECK(hipMemcpyAsync(out, d_out, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(wait_stream(st));
    return 0;
}

}  // namespace mlmc

using namespace mlmc;

extern "C" {

int mlmc_student_t_cdf(double dof, int64_t n, const double *y, double *u_out, int mem_kind) {
    MLMC_API_GUARD;
    return t_elementwise("mlmc_student_t_cdf", T_CDF, dof, n, y, u_out, mem_kind);
}

int mlmc_student_t_quantile(double dof, int64_t n, const double *p, double *y_out, int mem_kind) {
    MLMC_API_GUARD;
    return t_elementwise("mlmc_student_t_quantile", T_QUANTILE, dof, n, p, y_out, mem_kind);
}

int mlmc_chi2_mixing_scale(double dof, int64_t n, const double *p, double *s_out, int mem_kind) {
    MLMC_API_GUARD;
    return t_elementwise("mlmc_chi2_mixing_scale", T_CHI2, dof, n, p, s_out, mem_kind);
}

int mlmc_chi2_conditional_scale(double dof_mix, int64_t n, const double *p, double *s_out, int mem_kind) {
    MLMC_API_GUARD;
    return t_elementwise("mlmc_chi2_conditional_scale", T_CHI2, dof_mix, n, p, s_out, mem_kind, TCOP_MAX_DOF_MIX, "dof_mix");
}

}  // extern "C"
