// The max-entropy density on the device: the one place where its arithmetic is written (the kernels are in density.hip).
//
//     density(x) = exp(clip(-sum_r c_r Q_r(x), +-200)),   c = effective coefficients in the underlying (scaled) family
//
// A value outside the basis' domain (transform_value's keep flag) gives NaN.  Every sum has a fixed order, so a value depends
// on (basis, c, x) alone: not on the kernel that asks for it, not on the batch.
#pragma once
#include <type_traits>

#include "device_basis.hpp"

namespace mlmc {

// one density problem of a call
struct QProb {
    BasisParams bp;
    int n_coef;
    int64_t c_off;       // effective coefficients: coef + c_off, [n_coef]
    int64_t x_off, n;    // the problem's points: [x_off, x_off + n) of the call's point arrays
    double a, b;         // domain (0, 0 in the entries that take none: they do not read it)
};

// the run-time basis kind as a compile-time one: f(std::integral_constant<int, KIND>()), `decltype(K)::value` in a generic lambda
template <class F>
__device__ __forceinline__ auto with_kind(int kind, F &&f) {
    switch (kind) {
        case MLMC_LEGENDRE: return f(std::integral_constant<int, MLMC_LEGENDRE>());
        case MLMC_MONOMIAL: return f(std::integral_constant<int, MLMC_MONOMIAL>());
        case MLMC_FOURIER: return f(std::integral_constant<int, MLMC_FOURIER>());
        default: return f(std::integral_constant<int, MLMC_SPLINE>());
    }
}

// the chain of operations behind one density value: begin, term(r, c_r) for r = 0, 1, 2, ... in order, value
template <int KIND>
struct DensityChain {
    TermGen<KIND> g;
    double power;
    bool keep;
    __device__ __forceinline__ void begin(const BasisParams &bp, double x) {
        const double t = transform_value(bp, x, keep);
        g.init(keep ? t : 0.0, 1.0, bp);
        power = 0.0;
    }
    __device__ __forceinline__ void term(int r, double cr) { power = __builtin_fma(g.next(r), cr, power); }
    // the clipped exponent: what value() is the exp of
    __device__ __forceinline__ double exponent() const { return fmin(fmax(-power, -200.0), 200.0); }
    __device__ __forceinline__ double value() const { return keep ? exp(exponent()) : __builtin_nan(""); }
    // inside the basis' domain, and the sum is a number (NaN coefficients pass the clip as -200)
    __device__ __forceinline__ bool valid() const { return keep && power == power; }
};

template <int KIND>
__device__ __forceinline__ double density_value(const BasisParams &bp, const double *__restrict__ c, int R, double x) {
    DensityChain<KIND> d;
    d.begin(bp, x);
    for (int r = 0; r < R; ++r) d.term(r, c[r]);
    return d.value();
}

// density_value at two points at once: two chains interleaved term by term, so that one coefficient load serves both and one
// chain's FMAs overlap the other's.  Each chain is density_value's, hence so are its bits.
template <int KIND>
__device__ __forceinline__ void density_value2(const BasisParams &bp, const double *__restrict__ c, int R, double x0, double x1,
                                               double &d0, double &d1) {
    DensityChain<KIND> c0, c1;
    c0.begin(bp, x0);
    c1.begin(bp, x1);
    for (int r = 0; r < R; ++r) {
        const double cr = c[r];
        c0.term(r, cr);
        c1.term(r, cr);
    }
    d0 = c0.value();
    d1 = c1.value();
}

// clipped exponents e and densities rho = exp(e) (the bits of density_value) at N points at once: density_value2's interleaving of
// N chains; ok is cleared where a chain is not valid()
template <int KIND, int N>
__device__ __forceinline__ void density_exponents(const BasisParams &bp, const double *__restrict__ c, int R, const double (&x)[N],
                                                  double (&e)[N], double (&rho)[N], bool &ok) {
    DensityChain<KIND> ch[N];
#pragma unroll
    for (int i = 0; i < N; ++i) ch[i].begin(bp, x[i]);
    for (int r = 0; r < R; ++r) {
        const double cr = c[r];
#pragma unroll
        for (int i = 0; i < N; ++i) ch[i].term(r, cr);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        e[i] = ch[i].exponent();
        rho[i] = ch[i].value();
        ok = ok && ch[i].valid();
    }
}

// integral of the density over [a, b] with a `deg`-point Gauss-Legendre rule (nodes / weights on [-1, 1])
template <int KIND>
__device__ __forceinline__ double density_integral(const BasisParams &bp, const double *__restrict__ c, int R, double a, double b,
                                                   const double *__restrict__ nodes, const double *__restrict__ wts, int deg) {
    const double half = 0.5 * (b - a), mid = 0.5 * (b + a);
    double acc = 0.0;
    for (int k = 0; k < deg; ++k) acc = __builtin_fma(wts[k], density_value<KIND>(bp, c, R, __builtin_fma(half, nodes[k], mid)), acc);
    return acc * half;
}

// density_integral over [a0, b0] and over [a1, b1] at once: node k of both in one step through density_value2, so that the two
// chains of a node overlap.  Each integral is density_integral's chain of operations, hence so are its bits.
template <int KIND>
__device__ __forceinline__ void density_integral2(const BasisParams &bp, const double *__restrict__ c, int R, double a0, double b0,
                                                  double a1, double b1, const double *__restrict__ nodes,
                                                  const double *__restrict__ wts, int deg, double &i0, double &i1) {
    const double half0 = 0.5 * (b0 - a0), mid0 = 0.5 * (b0 + a0), half1 = 0.5 * (b1 - a1), mid1 = 0.5 * (b1 + a1);
    double acc0 = 0.0, acc1 = 0.0;
    for (int k = 0; k < deg; ++k) {
        double d0, d1;
        density_value2<KIND>(bp, c, R, __builtin_fma(half0, nodes[k], mid0), __builtin_fma(half1, nodes[k], mid1), d0, d1);
        acc0 = __builtin_fma(wts[k], d0, acc0);
        acc1 = __builtin_fma(wts[k], d1, acc1);
    }
    i0 = acc0 * half0;
    i1 = acc1 * half1;
}

}  // namespace mlmc
