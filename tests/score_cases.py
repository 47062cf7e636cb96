"""The normal scores of stored samples (include/mlmc_hip.h, mlmc_density_scores_batch) restated on the host, the closed-form
marginals and the copula case shared by tests/test_normal_scores_cpu.py and tests/test_gpu_normal_scores.py.  Nothing here touches
the device.

Closed-form marginals: rho(t) ~ exp(-r t) on t in [-1, 1], t = 2 (x - a) / (b - a) - 1, exactly a max-entropy density with the two
Legendre moments 1, t and the multipliers (lambda_0, r).  With E = expm1(-2 r),
    F(x) = expm1(-r (t + 1)) / E,    Q(p) = a + (b - a) (-log1p(p E) / r) / 2,    r = 0: F = (t + 1) / 2, the uniform."""
import numpy as np
from scipy import special

from tests import joint_sample_cases as jc

U = jc.U
U_LO, U_HI = jc.U_LO, jc.U_HI

# The largest error of the device's normcdfinv at the clamped uniforms of the points of tests/test_gpu_normal_scores.py::
# test_scores_against_mpmath (it prints it), against mpmath at 50 digits, in units of 2^-53 max(1, |z|).  The arguments are
# arbitrary doubles in [2^-53, 1 - 2^-53], not the odd multiples of 2^-53 behind jc.Z_UNITS_OBSERVED.  The tolerance is 4 x that
# rounded up to a power of two, at most 2^13 units (jc.tolerance).
Z_UNITS_OBSERVED = 4.251         # MI355X, ROCm device library normcdfinv, at u = 0.999990944200558; measured 2026-10-19 (tolerance 32)


def z_tolerance():
    return jc.tolerance(Z_UNITS_OBSERVED)


RATES = (5.0, -5.0, 0.0)
DOMAINS = ((-1.0, 1.0), (0.5, 4.5), (-3.0, 7.0))                 # the reference interval itself and two mapped ones
CORR = np.array([[1.0, 0.8, 0.5], [0.8, 1.0, 0.3], [0.5, 0.3, 1.0]])     # latent; the (5, -5) pair at 0.8
N_COPULA = 16384
FIRSTS = (0, 2 ** 33 + 1)
SEED = 0x9E3779B97F4A7C15


def multipliers(rate):
    """(lambda_0, lambda_1) of exp(-lambda_0 - rate t) with unit mass over t in [-1, 1]"""
    mass = 2.0 if rate == 0.0 else -np.expm1(-2.0 * rate) * np.exp(rate) / rate
    return np.array([np.log(mass), rate])


def closed_distribution(rate, domain, quad=(64, 21)):
    """the closed-form marginal as a distribution object with its multipliers set (no solve, no device work)"""
    import mlmc_amd
    from mlmc_amd.tool import simple_distribution as sd
    d = sd.SimpleDistribution(mlmc_amd.Legendre(2, domain), np.stack([np.eye(2)[0], np.ones(2)], axis=1), domain=domain)
    d.multipliers, d._moment_errs = multipliers(rate), np.ones(2)
    d.n_intervals, d._gauss_degree = quad
    return d


def closed_cdf(rate, domain, x):
    a, b = domain
    t1 = 2.0 * (np.asarray(x, dtype=np.float64) - a) / (b - a)                        # t + 1
    return 0.5 * t1 if rate == 0.0 else np.expm1(-rate * t1) / np.expm1(-2.0 * rate)


def closed_quantile(rate, domain, p):
    a, b = domain
    p = np.asarray(p, dtype=np.float64)
    t1 = 2.0 * p if rate == 0.0 else -np.log1p(p * np.expm1(-2.0 * rate)) / rate
    return a + 0.5 * (b - a) * t1


def twin_scores(cdf, domain, x):
    """the definition of the header in NumPy for one component with the CDF `cdf`: (z, u); NaN for NaN and outside the OPEN domain"""
    x = np.asarray(x, dtype=np.float64)
    keep = (x > domain[0]) & (x < domain[1])                                          # False for NaN
    u = np.full(x.shape, np.nan)
    u[keep] = cdf(x[keep])
    z = np.full(x.shape, np.nan)
    z[keep] = special.ndtri(np.minimum(np.maximum(u[keep], U_LO), U_HI))
    return z, u


def copula_case(first, factor):
    """(x [3, n], latent scores y [3, n]) of the copula case: y = F z with the bit-reproducible normals of jc.normals, x_m =
    Q_m(Phi(y_m)) in closed form"""
    z = jc.normals(SEED, range(3), first, N_COPULA)
    y = np.asarray(factor) @ z
    x = np.array([closed_quantile(r, d, special.ndtr(row)) for r, d, row in zip(RATES, DOMAINS, y)])
    return x, y


def standard_errors(values, corr):
    """|sample correlation of the rows - rho| in standard errors (1 - rho^2) / sqrt(n), upper triangle in row order"""
    n = values.shape[1]
    r = np.corrcoef(values)
    iu = np.triu_indices(corr.shape[0], 1)
    return np.abs(r[iu] - corr[iu]) / ((1.0 - corr[iu] ** 2) / np.sqrt(n))


def correlation_errors(corr_est, corr, n):
    """the same for a correlation matrix that has been estimated from n samples"""
    iu = np.triu_indices(corr.shape[0], 1)
    return np.abs(np.asarray(corr_est)[iu] - corr[iu]) / ((1.0 - corr[iu] ** 2) / np.sqrt(n))
