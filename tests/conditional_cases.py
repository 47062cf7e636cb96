"""The conditional law of a Gaussian copula (include/mlmc_hip.h, mlmc_density_sample_conditional_batch; tool.simple_distribution.
conditional_factor / conditional_samples / conditional_quantiles / conditional_cdfs) restated on the host, shared by
tests/test_conditional_cpu.py and tests/test_gpu_conditional_samples.py.  Nothing here touches the device.

With the correlation C of the normal scores, O the observed components and U the others (both ascending), the scores of U given
z_O are normal with mean C_UO C_OO^-1 z_O and covariance C_UU - C_UO C_OO^-1 C_OU: the textbook Schur complement, here in long
double by a Cholesky solve written out (NumPy's linalg has no long double).  The single-component law is N(mu_m, s_m^2), so the
conditional quantile at p is Q_m(p') with p' = Phi(mu + s Phi^-1(p)): restated with mpmath."""
import mpmath
import numpy as np

from tests import joint_sample_cases as jc

LD = np.longdouble
U = jc.U

# The largest error of the host map p -> p' = ndtr(mu + s ndtri(p)) (SciPy) against mpmath that tests/test_conditional_cpu.py has
# observed (it prints it), in units of 2^-53 max(p', 2^-53) over MAP_MU x MAP_S x MAP_P; the tolerance is jc.tolerance of it.
MAP_MU = (0.0, 1.0, -1.0, 3.0, -3.0)
MAP_S = (1.0, 0.6, 0.05)
MAP_P = np.concatenate([[1e-12, 1e-9, 1e-6, 1e-3], np.linspace(0.01, 0.99, 99), [1 - 1e-3, 1 - 1e-6, 1 - 1e-9, 1 - 1e-12]])
MAP_UNITS_OBSERVED = 140.6       # at (mu, s, p) = (-1, 1, 1e-12): y = -8.03, where half an ulp of y moves Phi(y) by 64 units
# The largest |conditional_cdfs(conditional_quantiles(p)) - p| that tests/test_gpu_conditional_samples.py has observed (it prints
# it), in units of 2^-53, over p in [0.01, 0.99], three sets and two components; next to it the test prints what the long-double
# Fhat of qc.RuleTable at the same quantiles pushed through the same map gives (4 units): the resolution of the quantile itself
ROUNDTRIP_UNITS_OBSERVED = 3.0   # MI355X

# the observed sets and scores of the statistics tests on jc.CORR3
STAT_CASES = (((0,), (1.2,)), ((2,), (-0.7,)), ((1, 2), (0.5, -1.5)))


def ld_cholesky(a):
    """lower Cholesky factor of a symmetric positive definite long-double matrix"""
    a = np.array(a, dtype=LD)
    n = a.shape[0]
    low = np.zeros((n, n), dtype=LD)
    for i in range(n):
        for j in range(i + 1):
            s = a[i, j] - np.dot(low[i, :j], low[j, :j])
            low[i, j] = np.sqrt(s) if i == j else s / low[j, j]
    return low


def ld_solve_spd(a, b):
    """a^-1 b for a symmetric positive definite a, in long double"""
    low = ld_cholesky(a)
    b = np.array(b, dtype=LD).reshape(a.shape[0], -1)
    y = np.zeros_like(b)
    for i in range(a.shape[0]):
        y[i] = (b[i] - low[i, :i] @ y[:i]) / low[i, i]
    x = np.zeros_like(b)
    for i in reversed(range(a.shape[0])):
        x[i] = (y[i] - low[i + 1:, i] @ x[i + 1:]) / low[i, i]
    return x


def schur(corr, observed):
    """(W [q, p], S [q, q], unobserved): W = C_UO C_OO^-1 and S = C_UU - C_UO C_OO^-1 C_OU of the long-double matrix `corr`"""
    c = np.array(corr, dtype=LD)
    M = c.shape[0]
    obs = np.array(sorted(observed), dtype=np.int64)
    unobs = np.setdiff1d(np.arange(M), obs)
    if obs.size == 0:
        return np.zeros((M, 0), dtype=LD), c, unobs
    c_oo, c_uo, c_uu = c[np.ix_(obs, obs)], c[np.ix_(unobs, obs)], c[np.ix_(unobs, unobs)]
    w = ld_solve_spd(c_oo, c_uo.T).T
    return w, c_uu - w @ c_uo.T, unobs


def used_correlation(factor):
    """F F^T in long double: the matrix C' that conditional_factor conditions"""
    f = np.asarray(factor, dtype=LD)
    return f @ f.T


def conditional_mean(w, z_obs):
    """mu [B, q] = (W z_O)^T for z_O [p, B], in long double"""
    return (np.asarray(w, dtype=LD) @ np.asarray(z_obs, dtype=LD).reshape(np.shape(w)[1], -1)).T


def mp_map(p, mu, s):
    """p' = Phi(mu + s Phi^-1(p)) at the fp64 numbers p in (0, 1), 50 digits; a list of mpf"""
    with mpmath.workdps(jc.MP_DIGITS):
        m, sd = mpmath.mpf(float(mu)), mpmath.mpf(float(s))
        return [mpmath.ncdf(m + sd * mpmath.sqrt(2) * mpmath.erfinv(2 * mpmath.mpf(float(v)) - 1)) for v in np.ravel(p)]


def map_units(got, ref):
    """|got - ref| in units of 2^-53 max(ref, 2^-53), ref a list of mpf"""
    with mpmath.workdps(jc.MP_DIGITS):
        lo = mpmath.mpf(U)
        return np.array([float(abs(mpmath.mpf(float(a)) - r) / (U * max(r, lo))) for a, r in zip(np.ravel(got), ref)])


def random_corr(rng, M):
    """a random positive definite correlation matrix"""
    a = rng.standard_normal((M, M + 3))
    c = a @ a.T
    d = 1.0 / np.sqrt(np.diag(c))
    c = c * d[:, None] * d[None, :]
    np.fill_diagonal(c, 1.0)
    return 0.5 * (c + c.T)


def score_statistics(scores, mu, fc):
    """of rows of conditional scores [q, n] that should be N(mu, F_c F_c^T): (|mean - mu| in standard errors s / sqrt(n),
    |variance - s^2| in standard errors s^2 sqrt(2 / (n - 1)), |correlation - rho| in standard errors (1 - rho^2) / sqrt(n - 1) of
    the conditional correlation rho, Kolmogorov distance of Phi((score - mu) / s) from uniform), each the largest over the rows"""
    from scipy import special
    from tests import sample_cases as sc
    scores = np.asarray(scores)
    q, n = scores.shape
    cov = np.asarray(fc) @ np.asarray(fc).T
    s = np.sqrt(np.diag(cov))
    mean = np.max(np.abs(scores.mean(axis=1) - mu) / (s / np.sqrt(n)))
    var = np.max(np.abs(scores.var(axis=1, ddof=1) - s * s) / (s * s * np.sqrt(2.0 / (n - 1))))
    corr = 0.0
    if q > 1:
        corr = float(np.max(jc.correlation_errors(scores, cov / s[:, None] / s[None, :])))
    ks = max(sc.kolmogorov_distance(special.ndtr((row - m) / sd)) for row, m, sd in zip(scores, mu, s))
    return float(mean), float(var), corr, float(ks)
