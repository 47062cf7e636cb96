"""The Student-t copula entries (include/mlmc_hip.h: mlmc_student_t_cdf, mlmc_chi2_mixing_scale,
mlmc_density_sample_joint_t_batch) restated on the host, shared by tests/test_t_copula_cpu.py and tests/test_gpu_t_copula.py.
Nothing here touches the device.

  * the mixing uniform p0 of draw j (Philox: tests/sample_cases.py, Sobol': tests/sobol_cases.py)
  * references at 50 digits: T_nu through mpmath.betainc, the chi-square CDF through mpmath.gammainc (both regularised)
  * the TWIN: the algorithm of mlmc_amd/csrc/copula_t.hip in Python floats, statement by statement, which also counts the trips
    of every capped loop (the device code cannot report them)
  * the units of the two functions and the largest errors observed"""
import math

import mpmath
import numpy as np
from scipy import special

from tests import joint_sample_cases as jc
from tests import sample_cases as sc

U = 2.0 ** -53
MP_DIGITS = 50
DOFS = (1.0, 1.5, 2.0, 3.0, 4.5, 8.0, 30.0, 64.0)

# the caps of copula_t.hip
T_SERIES_CAP = 200
T_LENTZ_CAP = 200
C_SERIES_CAP = 400
C_LENTZ_CAP = 400
C_NEWTON_CAP = 40

# The largest errors observed against mpmath, in the units of t_units / s_units: of the twin on this file's arguments (CPU test,
# printed with -s) and of the device functions (tests/test_gpu_t_copula.py prints them).  The tolerances are
# joint_sample_cases.tolerance(observed): 4 x observed rounded up to a power of two, at most 2^13.
T_UNITS_OBSERVED_TWIN = 57.98   # nu = 64 at y = -1.2, the first value of the continued fraction
S_UNITS_OBSERVED_TWIN = 20.21   # nu = 64 at p = 0.567
T_UNITS_OBSERVED = 57.98         # MI355X: nu = 64 at y = -1.2; per nu 3.1, 8.9, 6.7, 6.4, 11.5, 20.3, 46.3, 58.0
S_UNITS_OBSERVED = 20.2          # MI355X: nu = 64 at p = 0.567; per nu 11.7, 9.5, 8.5, 6.9, 8.6, 4.6, 13.6, 20.2


class Constants:
    """tcop_constants of copula_t.hip"""

    def __init__(self, dof):
        self.dof = float(dof)
        self.sqrt_dof = math.sqrt(dof)
        self.A = 0.5 * (dof + 1.0)
        with mpmath.workdps(30):                      # the library forms it in long double
            nu = mpmath.mpf(self.dof)
            self.c0 = float(mpmath.gamma((nu + 1) / 2) / (mpmath.sqrt(nu * mpmath.pi) * mpmath.gamma(nu / 2)))
            self.lg_a1 = float(mpmath.loggamma(nu / 2 + 1))
        self.t_split = min(1.2, self.sqrt_dof)
        self.a = 0.5 * dof


class Trips:
    """the largest trip count of every capped loop, and how often a cap was reached"""

    def __init__(self):
        self.t_series = self.t_lentz = self.c_series = self.c_lentz = self.c_newton = 0
        self.capped = 0

    def note(self, name, trips, cap, converged):
        setattr(self, name, max(getattr(self, name), trips))
        if not converged:
            self.capped += 1
        assert trips <= cap


def _t_series(A, B, z, trips):
    term, total = 1.0, 1.0
    done = False
    n = 0
    for n in range(T_SERIES_CAP):
        term *= z * ((A + n) / (B + n))
        total += term
        if term <= total * 2.0 ** -56:
            done = True
            break
    trips.note("t_series", n + 1, T_SERIES_CAP, done)
    return total


def _t_fraction(a, x, trips):
    """the continued fraction of I_x(a, 1/2) (modified Lentz), which stands for the tail series where that is slow"""
    tiny = 2.0 ** -1000
    qab, qap, qam = a + 0.5, a + 1.0, a - 1.0
    c = 1.0
    d = 1.0 - qab * x / qap
    if abs(d) < tiny:
        d = tiny
    d = 1.0 / d
    h = d
    done = False
    m = 1
    for m in range(1, T_LENTZ_CAP + 1):
        m2 = 2.0 * m
        aa = m * (0.5 - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        if abs(d) < tiny:
            d = tiny
        c = 1.0 + aa / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        if abs(d) < tiny:
            d = tiny
        c = 1.0 + aa / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        dl = d * c
        h *= dl
        if abs(dl - 1.0) <= 2.0 ** -50:
            done = True
            break
    trips.note("t_lentz", m, T_LENTZ_CAP, done)
    return h


def _pow(r, e):
    try:
        return math.pow(r, e)
    except OverflowError:
        return math.inf


def twin_t_lower(C, t, trips):
    """T_nu(-t), t >= 0"""
    if t < C.t_split:
        q = t * t / C.dof
        w = q / (1.0 + q)
        pre = t * C.c0 * math.exp(-C.A * math.log1p(q))
        return 0.5 - pre * _t_series(C.A, 1.5, w, trips)
    if t == math.inf:
        return 0.0
    if t < C.sqrt_dof:
        q = t * t / C.dof
        w = q / (1.0 + q)
        pre = (C.c0 / C.sqrt_dof) * math.exp(-C.a * math.log1p(q)) * math.sqrt(w)
        return pre * _t_fraction(C.a, 1.0 / (1.0 + q), trips)
    r = C.sqrt_dof / t
    q = r * r
    pre = (C.c0 / C.sqrt_dof) * _pow(r, C.dof) * math.exp(-C.A * math.log1p(q))
    return pre * _t_series(C.A, C.a + 1.0, q / (1.0 + q), trips)


def twin_t_cdf(C, y, trips):
    if y != y:
        return y
    return twin_t_lower(C, -y, trips) if y <= 0.0 else 1.0 - twin_t_lower(C, y, trips)


def _gamma_pq(C, x, trips):
    a = C.a
    D = math.exp(a * math.log(x) - x - C.lg_a1)
    if x < a + 1.0:
        term, total = 1.0, 1.0
        done = False
        n = 0
        for n in range(C_SERIES_CAP):
            term *= x / (a + 1.0 + n)
            total += term
            if term <= total * 2.0 ** -56:
                done = True
                break
        trips.note("c_series", n + 1, C_SERIES_CAP, done)
        P = D * total
        return P, 1.0 - P, D
    tiny = 2.0 ** -1000
    b = x + 1.0 - a
    c = 1.0 / tiny
    d = 1.0 / b
    h = d
    done = False
    i = 1
    for i in range(1, C_LENTZ_CAP + 1):
        an = -float(i) * (float(i) - a)
        b += 2.0
        d = an * d + b
        if abs(d) < tiny:
            d = tiny
        c = b + an / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        dl = d * c
        h *= dl
        if abs(dl - 1.0) <= 2.0 ** -50:
            done = True
            break
    trips.note("c_lentz", i, C_LENTZ_CAP, done)
    Q = a * D * h
    return 1.0 - Q, Q, D


def twin_chi2_scale(C, p, trips):
    if not 0.0 < p < 1.0:
        return math.nan
    a = C.a
    lower = p <= 0.5
    target = p if lower else 1.0 - p
    c9 = 1.0 / (9.0 * a)
    wh = 1.0 - c9 + float(special.ndtri(p)) * math.sqrt(c9)
    x_small = math.exp((math.log(p) + C.lg_a1) / a)
    x = a * wh * wh * wh
    if not wh > 0.0 or x_small < 0.2 * (a + 1.0):
        x = x_small
    done = False
    it = 0
    for it in range(C_NEWTON_CAP):
        P, Q, D = _gamma_pq(C, x, trips)
        v = P if lower else Q
        rel = (v - target) / target
        h = math.log1p(rel) if abs(rel) < 0.5 else math.log(v / target)
        if lower:
            step = min(max(-h * P / (a * D), -3.0), 3.0)
            x *= math.exp(step)
        else:
            step = min(max(h * Q / (a * D), -0.5), 1.0)
            x += x * step
        if abs(step) <= 2.0 ** -30:
            done = True
            break
    trips.note("c_newton", it + 1, C_NEWTON_CAP, done)
    return math.sqrt(a / x)


# ---- arguments -------------------------------------------------------------------------------------------------------------

def _ulp_neighbours(v):
    return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]


def t_arguments(dof):
    """the y of the accuracy tests for one nu: the listed magnitudes of both signs, 2000 log-spaced magnitudes of both signs and
    the thresholds where the implementation switches formula (0, +-t_split and +-sqrt(nu)), one ulp to either side"""
    C = Constants(dof)
    mags = [1e-300, 1e-8, 0.1, 0.5, 1.0, math.sqrt(dof), 2.0, 5.0, 10.0, 1e2, 1e4, 1e8, 1e16, 1e300]
    mags += list(10.0 ** np.linspace(-300.0, 300.0, 2000))
    for v in _ulp_neighbours(C.t_split) + _ulp_neighbours(C.sqrt_dof):
        mags.append(float(v))
    mags.append(5e-324)                               # one ulp to either side of 0
    mags = np.array(mags)
    return np.concatenate([[0.0], -mags, mags])


def p_arguments():
    fixed = [U, 2.0 ** -30, 1e-6, 0.01, 0.5, 0.99, 1.0 - 1e-9, 1.0 - U, np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0)]
    return np.concatenate([fixed, sc.stream_uniforms(7, 5, np.arange(2000, dtype=np.uint64))])


# ---- references ------------------------------------------------------------------------------------------------------------

def mp_t_lower(dof, t):
    """T_nu(-t) for the fp64 magnitudes t >= 0, a list of mpf: I_x(nu/2, 1/2) / 2, x = nu / (nu + t^2), in the tail and
    1/2 - I_w(1/2, nu/2) / 2, w = 1 - x, at the centre, both without cancellation"""
    out = []
    with mpmath.workdps(MP_DIGITS):
        nu = mpmath.mpf(float(dof))
        for v in np.ravel(t):
            tt = mpmath.mpf(float(v))
            if tt * tt < nu:
                w = tt * tt / (nu + tt * tt)
                out.append((1 - mpmath.betainc(mpmath.mpf(1) / 2, nu / 2, 0, w, regularized=True)) / 2)
            else:
                x = nu / (nu + tt * tt)
                out.append(mpmath.betainc(nu / 2, mpmath.mpf(1) / 2, 0, x, regularized=True) / 2)
    return out


def mp_t_cdf(dof, y):
    """T_nu at the fp64 numbers y, a list of mpf (the magnitudes are evaluated once)"""
    y = np.ravel(np.asarray(y, dtype=np.float64))
    mags, inv = np.unique(np.abs(y), return_inverse=True)
    low = mp_t_lower(dof, mags)
    with mpmath.workdps(MP_DIGITS):
        return [low[i] if v <= 0.0 else 1 - low[i] for v, i in zip(y, inv)]


def t_units(u, ref):
    """the units of the copula uniforms (joint_sample_cases.phi_units without the clamp): |u - T| / (2^-53 max(T, tiny)) for
    T <= 1/2, which is relative in the lower tail, and |u - T| / 2^-53 scaled by T >= 1/2 above, which is 2^-53 absolute.  A
    reference below the smallest normal number is compared in units of the smallest subnormal."""
    out = []
    with mpmath.workdps(MP_DIGITS):
        for a, r in zip(np.ravel(u), ref):
            scale = max(U * r, mpmath.mpf(2) ** -1074)
            out.append(float(abs(mpmath.mpf(float(a)) - r) / scale))
    return np.array(out)


def s_units(dof, p, s):
    """|P_nu(g) - p| / (2^-53 (min(p, 1 - p) + 2 g f_nu(g))) with g = nu / s^2: the second term is what the rounding of s moves"""
    out = []
    with mpmath.workdps(MP_DIGITS):
        a = mpmath.mpf(float(dof)) / 2
        for pv, sv in zip(np.ravel(p), np.ravel(s)):
            pm, sm = mpmath.mpf(float(pv)), mpmath.mpf(float(sv))
            g = 2 * a / (sm * sm)
            x = g / 2
            gf = x ** a * mpmath.exp(-x) / mpmath.gamma(a)           # g f_nu(g) = x^a e^-x / Gamma(a)
            if pv <= 0.5:
                err = abs(mpmath.gammainc(a, 0, x, regularized=True) - pm)
            else:
                err = abs(mpmath.gammainc(a, x, mpmath.inf, regularized=True) - (1 - pm))
            out.append(float(err / (U * (min(pm, 1 - pm) + 2 * gf))))
    return np.array(out)


# ---- the sampling entry ----------------------------------------------------------------------------------------------------

def mixing_uniforms(seed, mix_stream, first, n, antithetic=False, qmc=False):
    """p0 [n] of the draws first .. first + n - 1"""
    if qmc:
        from tests import sobol_cases
        return sobol_cases.uniforms(seed, mix_stream, first, n)
    j = np.uint64(first) + np.arange(n, dtype=np.uint64)
    i = j >> np.uint64(1) if antithetic else j
    return np.asarray(sc.stream_uniforms(seed, mix_stream, i), dtype=np.float64)


def clamp(u):
    return np.minimum(np.maximum(u, jc.U_LO), jc.U_HI)


# ---- the statistics of the draws ---------------------------------------------------------------------------------------------
# M = 3 components at concordance_cases.CORR, nu = 3, one level of 2^18 draws, latent normals on streams 0, 1, 2 and the mixing
# variable on stream 3.  NumPy draws of the same law gave |z| <= 2.0 under the t model and z >= 16 under the Gaussian model at 0.9.
STAT_DOF = 3.0
STAT_N = 2 ** 18
STAT_SEED = 20261020
STAT_PROBS = (0.5, 0.9, 0.95)
STAT_Z_BOUND = 5.0               # |z| under the t model, every pair and level
STAT_Z_GAUSS = 8.0               # z under the Gaussian model at p = 0.9, every pair
STAT_SOBOL_SEEDS = tuple(range(8))
STAT_SOBOL_N = 2 ** 15


def concordance_z(pair, kept, probs=STAT_PROBS, dof=STAT_DOF, corr=None):
    """one level of counts pair [G, 3, M, M] (events u > p_g) of `kept` draws -> dict(prob, var, z_t [G, pairs] against the t orthant,
    z_gauss against the normal orthant, fit: fit_copula_dof on the levels above 1/2), all at `corr` (None: concordance_cases.CORR)"""
    from mlmc_amd.tool import simple_distribution as sd
    from tests import concordance_cases as cc
    corr = cc.CORR if corr is None else np.clip(np.asarray(corr, dtype=np.float64), -1.0, 1.0)      # F F^T has a diagonal of 1 + rounding
    _, _, prob, var = cc.twin_level_statistics(np.array([int(kept)]), np.asarray(pair)[None])
    p = np.asarray(probs, dtype=np.float64)
    h = special.stdtrit(dof, p)[:, None, None]
    z_t = cc.off_diagonal(cc.z_scores(prob, var, sd.bivariate_t_orthant(h, h, corr[None], dof)))
    z_gauss = cc.off_diagonal(cc.z_scores(prob, var, cc.model_orthant(p, corr)))
    tail = p > 0.5
    return dict(prob=prob, var=var, z_t=z_t, z_gauss=z_gauss, fit=sd.fit_copula_dof(prob[tail], var[tail], p[tail], corr))
