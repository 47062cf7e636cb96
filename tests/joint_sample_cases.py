"""The latent normals and copula uniforms of the joint sampling entry (include/mlmc_hip.h, mlmc_density_sample_joint_batch)
restated on the host, shared by tests/test_joint_samples_cpu.py and tests/test_gpu_joint_samples.py.  Nothing here touches the
device.

Latent normal k of draw j: z = Phi^-1(uniform i of stream streams[k]) with the uniforms of tests/sample_cases.py, i = j, or with
the antithetic flag i = j >> 1 and z negated for odd j.  y = F z, u = min(max(Phi(y), 2^-53), 1 - 2^-53)."""
import mpmath
import numpy as np
from scipy import special

from tests import sample_cases as sc

LD = np.longdouble
U = 2.0 ** -53
U_LO, U_HI = U, 1.0 - U
MP_DIGITS = 50

# The largest errors of the device's normcdfinv and normcdf that tests/test_gpu_joint_samples.py has observed against mpmath (it
# prints them), in the units of z_units / phi_units; the tolerances are 4 x that rounded up to a power of two (the margin covers
# inputs that are not in the sample), and at most 2^-40 relative = 2^13 units: a wrong stream, index or word order is an O(1) error.
Z_UNITS_OBSERVED = 3.416         # MI355X, ROCm device library normcdfinv; 3.81 over 20 000 further normals
PHI_UNITS_OBSERVED = 3.195       # normcdf; 3.58 over 20 000 further values
UNITS_CAP = 2.0 ** 13


def tolerance(observed):
    """4 x observed, rounded up to a power of two, at most UNITS_CAP"""
    tol = 2.0 ** int(np.ceil(np.log2(4.0 * max(observed, 2.0 ** -10))))
    assert tol <= UNITS_CAP, (observed, tol)
    return tol


def z_tolerance():
    return tolerance(Z_UNITS_OBSERVED)


def phi_tolerance():
    """E_Phi in the units of phi_units"""
    return tolerance(PHI_UNITS_OBSERVED)


def latent_uniforms(seed, streams, first, n, antithetic=False):
    """[K, n]: the uniform behind latent normal k of the draws first .. first + n - 1, and the mask of the draws whose normal is negated"""
    j = np.uint64(first) + np.arange(n, dtype=np.uint64)
    i = j >> np.uint64(1) if antithetic else j
    u0 = np.array([sc.stream_uniforms(seed, s, i) for s in streams], dtype=np.float64).reshape(len(streams), n)
    neg = (j & np.uint64(1)).astype(bool) if antithetic else np.zeros(n, dtype=bool)
    return u0, neg


def normals(seed, streams, first, n, antithetic=False):
    """[K, n] latent normals through scipy.special.ndtri"""
    u0, neg = latent_uniforms(seed, streams, first, n, antithetic)
    z = special.ndtri(u0)
    return np.where(neg[None, :], -z, z)


def mp_ndtri(u):
    """Phi^-1 at the fp64 numbers u in (0, 1), 50 digits; a list of mpf"""
    with mpmath.workdps(MP_DIGITS):
        return [mpmath.sqrt(2) * mpmath.erfinv(2 * mpmath.mpf(float(v)) - 1) for v in np.ravel(u)]


def mp_ncdf(y):
    """Phi at the numbers y (fp64 or long double), 50 digits; a list of mpf"""
    with mpmath.workdps(MP_DIGITS):
        return [mpmath.ncdf(_mpf(v)) for v in np.ravel(y)]


def _mpf(v):
    """a long double as an mpf without loss: high part + remainder"""
    hi = float(v)
    return mpmath.mpf(hi) + mpmath.mpf(float(LD(v) - LD(hi)))


def z_units(z, ref):
    """|z - ref| in units of 2^-53 max(1, |ref|), ref a list of mpf"""
    with mpmath.workdps(MP_DIGITS):
        return np.array([float(abs(mpmath.mpf(float(a)) - r) / (U * max(1, abs(r)))) for a, r in zip(np.ravel(z), ref)])


def phi_units(u, ref):
    """|u - clamp(ref)| in units of 2^-53 max(ref, 2^-53), ref = Phi as a list of mpf"""
    with mpmath.workdps(MP_DIGITS):
        lo, hi = mpmath.mpf(U_LO), mpmath.mpf(U_HI)
        return np.array([float(abs(mpmath.mpf(float(a)) - min(max(r, lo), hi)) / (U * max(r, lo))) for a, r in zip(np.ravel(u), ref)])


def phi_abs_errors(u, ref):
    """|u - clamp(ref)| as fp64 numbers, ref = Phi as a list of mpf"""
    with mpmath.workdps(MP_DIGITS):
        lo, hi = mpmath.mpf(U_LO), mpmath.mpf(U_HI)
        return np.array([float(abs(mpmath.mpf(float(a)) - min(max(r, lo), hi))) for a, r in zip(np.ravel(u), ref)])


def ld_dot(F, z):
    """F z in long double, [M, n]"""
    return np.asarray(F, dtype=LD) @ np.asarray(z, dtype=LD)


def random_factor(rng, M, K):
    """[M, K] with rows of unit norm"""
    F = rng.standard_normal((M, K))
    return np.ascontiguousarray(F / np.sqrt(np.sum(F * F, axis=1))[:, None])


CORR3 = np.array([[1.0, 0.8, -0.5], [0.8, 1.0, -0.2], [-0.5, -0.2, 1.0]])     # eigenvalues 0.137, 0.822, 2.04


def correlation_errors(scores, corr):
    """|sample correlation - rho| of the rows of `scores` in standard errors (1 - rho^2) / sqrt(n - 1), off-diagonal entries"""
    n = scores.shape[1]
    r = np.corrcoef(scores)
    iu = np.triu_indices(corr.shape[0], 1)
    return np.abs(r[iu] - corr[iu]) / ((1.0 - corr[iu] ** 2) / np.sqrt(n - 1.0))
