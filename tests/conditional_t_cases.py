"""The conditional law of a Student-t copula (include/mlmc_hip.h, mlmc_density_sample_conditional_t_batch and
mlmc_chi2_conditional_scale; tool.simple_distribution.conditional_samples / conditional_quantiles / conditional_cdfs with dof)
restated on the host, shared by tests/test_conditional_t_cpu.py and tests/test_gpu_conditional_t.py.  Nothing here touches the
device.

With the copula's correlation C, O the p observed components and y_O their t scores, the t scores of the others are multivariate t
with nu + p degrees of freedom, location C_UO C_OO^-1 y_O and scale matrix g (C_UU - C_UO C_OO^-1 C_OU), g = (nu + d) / (nu + p),
d = y_O^T C_OO^-1 y_O.  Here:

  * L_OO, d and r = sqrt(g) in long double (the Cholesky solve of tests/conditional_cases.py)
  * the conditional CDF of ONE free t score by the DEFINITION, int_{-inf}^{y} f_nu(y_O, t) dt / f_nu(y_O) with the multivariate t
    density f_nu, through mpmath.quad: it uses none of the formulas above
  * T_nu^-1 at an fp64 probability in mpmath (a root of the regularised incomplete beta function)
  * the shapes of the GPU tests and the recorded numbers"""
import mpmath
import numpy as np

from tests import conditional_cases as cc
from tests import t_copula_cases as tc

LD = np.longdouble
U = tc.U

# the mixing variable of the conditional entry has nu + p degrees of freedom, up to 192; the other entries end at 64
MAX_DOF, MAX_DOF_MIX = 64.0, 192.0
WIDE_DOFS = (64.5, 96.5, 128.0, 192.0)

# The largest error of the mixing scale against mpmath in the units of t_copula_cases.s_units, per nu of WIDE_DOFS over the full
# t_copula_cases.p_arguments(): of the fp64 twin (tests/test_conditional_t_cpu.py prints it with -s) and of the device
# (tests/test_gpu_conditional_t.py prints it).  The GPU gate is joint_sample_cases.tolerance(max of the twin's): 4 x, rounded up to
# a power of two; the device's exp / log differ from NumPy's, which is what the factor covers.
S_UNITS_OBSERVED_TWIN_WIDE = {64.5: 21.71, 96.5: 39.93, 128.0: 30.12, 192.0: 59.23}     # at p = 0.572, 0.571, 0.564, 0.546
S_UNITS_OBSERVED_WIDE = {64.5: 21.71, 96.5: 39.93, 128.0: 30.12, 192.0: 59.23}          # MI355X: the twin's values, at the same p

# The largest absolute errors of the two host maps against the conditional CDF by the definition over map_cases() x
# conditional_cases.MAP_P (tests/test_conditional_t_cpu.py prints them): of simple_distribution._t_conditional_cdf_map, and of
# the inverse of _t_conditional_quantile_map.  The tolerance of each is 4 x its record, and never more than MAP_ABS_CAP.
MAP_ABS_OBSERVED = 2.959e-11            # nu = 1, rho = 0.9, y_O = (6, 6), p = 0.62: SciPy's stdtrit is good to about 1e-11 relative
MAP_INVERSE_ABS_OBSERVED = 7.443e-11    # nu = 30, rho = 0.9, y_O = (6, -6), p = 1 - 1e-9: p' = 1 - 5.6e-16, 2.5 ulps from 1 in fp64
MAP_ABS_CAP = 1e-9
MAP_DOFS = (1.0, 3.0, 30.0)
MAP_RHOS = (0.3, -0.3, 0.9)
MAP_SCORES = (0.0, 1.0, -1.0, 6.0, -6.0)
MAP_SCORE_PAIRS = ((0.0, 0.0), (1.0, 1.0), (1.0, -1.0), (-1.0, 0.0), (6.0, 6.0), (6.0, -6.0), (-6.0, 1.0))
MAP_DIGITS = 30

# the shapes of tests/test_gpu_conditional_t.py: they cross the 64-row tile, the 32-k panel and the 64-draw tile
REDUCTION_SHAPES = ((1, 1, 17, 0), (17, 5, 257, 3), (65, 65, 65, 0))                       # M, K, n, first
REDUCTION_DOFS = (1.0, 3.0, 64.0)
EPILOGUE_SHAPES = ((1, 1, 17, 1), (3, 3, 1000, 2), (17, 5, 257, 3), (65, 65, 65, 2), (16, 17, 64, 5))     # M, K, n, B
EPILOGUE_DOFS = ((3.0, 4.0), (1.5, 6.5), (64.0, 192.0))                                   # dof, dof_mix
STRUCTURE_SHAPE = (17, 5, 257, 5)
STAT_DOF = 3.0
STAT_N = 2 ** 16
STAT_PROBS = (0.05, 0.5, 0.95)
STAT_FAR = 0.999                 # the quantile of component 0 that the far set is given


def equicorrelation(M, rho):
    c = np.full((M, M), float(rho))
    np.fill_diagonal(c, 1.0)
    return c


def map_cases():
    """(corr, observed, y_O): M = 2 with component 0 observed and M = 3 with components 0 and 1 observed and one free"""
    out = []
    for rho in MAP_RHOS:
        out += [(equicorrelation(2, rho), (0,), (y,)) for y in MAP_SCORES]
        out += [(equicorrelation(3, rho), (0, 1), pair) for pair in MAP_SCORE_PAIRS]
    return out


def ld_observed(corr_used, observed, y_obs, dof):
    """(L_OO [p, p], d [B], r [B]) in long double for the long-double matrix `corr_used` (conditional_cases.used_correlation) and the
    t scores y_obs [p, B]: d = |L_OO^-1 y_O|^2, r = sqrt((nu + d) / (nu + p))"""
    obs = np.array(sorted(observed), dtype=np.int64)
    y = np.array(y_obs, dtype=LD).reshape(obs.size, -1)
    low = cc.ld_cholesky(np.array(corr_used, dtype=LD)[np.ix_(obs, obs)])
    v = np.zeros_like(y)
    for i in range(obs.size):
        v[i] = (y[i] - low[i, :i] @ v[:i]) / low[i, i]
    d = np.sum(v * v, axis=0)
    nu = LD(dof)
    return low, d, np.sqrt((nu + d) / (nu + LD(obs.size)))


def _mp_t_density(corr, dof):
    """(norm, C^-1, nu) of the multivariate t density f_nu(x) = norm (1 + x^T C^-1 x / nu)^(-(nu + M) / 2), in mpmath"""
    M = len(corr)
    c = mpmath.matrix([[mpmath.mpf(float(v)) for v in row] for row in corr])
    nu = mpmath.mpf(float(dof))
    norm = mpmath.gamma((nu + M) / 2) / (mpmath.gamma(nu / 2) * (nu * mpmath.pi) ** (mpmath.mpf(M) / 2) * mpmath.sqrt(mpmath.det(c)))
    return norm, c ** -1, nu


def mp_conditional_cdf(corr, y_obs, dof, y):
    """P(Y_last <= y | Y_O = y_obs) for a t vector with correlation `corr` whose first p components are observed and whose last is
    free, by the definition: int_{-inf}^{y} f_nu(y_O, t) dt / f_nu(y_O); y a list of mpf, the result a list of mpf.  The integral is
    taken in theta, t = peak + tan(theta), where the integrand is smooth up to theta = -pi / 2 (mpmath.quad's infinite intervals
    lose digits on an algebraic tail); `peak`, the regression of the free score on the observed ones, only places the break point.
    The last entry of the result is the whole integral over the marginal density, which is 1: the reference's own error."""
    corr = np.asarray(corr, dtype=np.float64)
    p = corr.shape[0] - 1
    with mpmath.workdps(MAP_DIGITS):
        yo = [mpmath.mpf(float(v)) for v in y_obs]
        norm, inv, nu = _mp_t_density(corr, dof)
        norm_o, inv_o, _ = _mp_t_density(corr[:p, :p], dof)
        den = norm_o * (1 + sum(yo[i] * inv_o[i, j] * yo[j] for i in range(p) for j in range(p)) / nu) ** (-(nu + p) / 2)
        # x^T C^-1 x for x = (y_O, t) as a polynomial in t
        q0 = sum(yo[i] * inv[i, j] * yo[j] for i in range(p) for j in range(p))
        q1 = sum(inv[i, p] * yo[i] for i in range(p))
        q2, power = inv[p, p], -(nu + p + 1) / 2
        peak = mpmath.mpf(float(np.linalg.solve(corr[:p, :p], corr[:p, p]) @ np.asarray(y_obs, dtype=np.float64)))
        half_pi = mpmath.pi / 2

        def g(theta):
            c = mpmath.cos(theta)
            if c == 0:
                return mpmath.mpf(0)
            t = peak + mpmath.sin(theta) / c
            return norm * (1 + (q0 + 2 * q1 * t + q2 * t * t) / nu) ** power / (c * c)
        # in theta the integrand is analytic on the closed interval (nu + M is an integer here): a FIXED Gauss-Legendre rule of 48
        # nodes on pieces of at most pi / 8, accumulated from -pi / 2 through the sorted arguments.  mpmath.quad's adaptive rules
        # stop too early on some of these integrals (errors up to 1e-8 against an estimate of 1e-30)
        nodes = _gl_nodes()

        def integral(lo, hi):
            pieces = max(1, int(mpmath.ceil((hi - lo) / (mpmath.pi / 8))))
            h, total = (hi - lo) / pieces / 2, mpmath.mpf(0)
            for k in range(pieces):
                mid = lo + (2 * k + 1) * h
                total += h * sum(wt * g(mid + h * x) for x, wt in nodes)
            return total / den
        thetas = [half_pi if v == mpmath.inf else -half_pi if v == -mpmath.inf else mpmath.atan(v - peak) for v in y]
        out, run, at = [None] * len(thetas), mpmath.mpf(0), -half_pi
        for k in sorted(range(len(thetas)), key=lambda i: thetas[i]):
            if thetas[k] > at:
                run += integral(at, thetas[k])
                at = thetas[k]
            out[k] = run
        return out + [run + (integral(at, half_pi) if at < half_pi else 0)]


_GL_NODES = {}


def _gl_nodes():
    """the 48 nodes and weights of a Gauss-Legendre rule on [-1, 1] at the working precision"""
    prec = mpmath.mp.prec
    if prec not in _GL_NODES:
        from mpmath.calculus.quadrature import GaussLegendre
        _GL_NODES[prec] = GaussLegendre(mpmath.mp).calc_nodes(5, prec)
    return _GL_NODES[prec]


def mp_t_quantile(dof, f, start):
    """T_nu^-1 at the fp64 probabilities f in (0, 1), a list of mpf: Newton on the lower tail of the nearer side from the fp64
    start values, at MAP_DIGITS digits"""
    out = []
    with mpmath.workdps(MAP_DIGITS):
        nu, half = mpmath.mpf(float(dof)), mpmath.mpf(1) / 2
        c0 = mpmath.gamma((nu + 1) / 2) / (mpmath.sqrt(nu * mpmath.pi) * mpmath.gamma(nu / 2))

        def lower(t):                                         # T_nu(-t)
            if t < 0:
                return 1 - lower(-t)
            if t * t < nu:
                return (1 - mpmath.betainc(half, nu / 2, 0, t * t / (nu + t * t), regularized=True)) / 2
            return mpmath.betainc(nu / 2, half, 0, nu / (nu + t * t), regularized=True) / 2
        for fv, s in zip(np.ravel(f), np.ravel(start)):
            if fv <= 0.0 or fv >= 1.0:
                out.append(-mpmath.inf if fv <= 0.0 else mpmath.inf)
                continue
            fm = mpmath.mpf(float(fv))
            upper = fm > half
            target = 1 - fm if upper else fm                  # exact
            t = abs(mpmath.mpf(float(s)))
            for _ in range(60):
                dens = c0 * (1 + t * t / nu) ** (-(nu + 1) / 2)
                step = (lower(t) - target) / dens             # d lower / dt = -density
                t += step
                if abs(step) <= mpmath.mpf(10) ** (-MAP_DIGITS + 4) * max(1, abs(t)):
                    break
            out.append(t if upper else -t)
    return out
