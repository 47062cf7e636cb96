"""The copula log-density entries (include/mlmc_hip.h: mlmc_student_t_quantile, mlmc_copula_log_density) restated on the host,
shared by tests/test_copula_lik_cpu.py, tests/test_gpu_copula_lik.py and tests/test_gpu_copula_lik_api.py.  Nothing here touches
the device.

  * the TWIN of the t quantile: the algorithm of mlmc_amd/csrc/copula_t.hip in Python floats, statement by statement, on
    tests/t_copula_cases.py's twin of t_lower; it counts the trips of the Halley loop (the device code cannot report them)
  * the TWIN of the chain of copula_lik.hip in NumPy fp64, one rounded operation at a time, in the kernel's order
  * references: the t quantile in mpmath at MP_DIGITS digits; the log density from given scores in long double (11 more bits; at
    M = 12 fewer than 2^7 operations per value), and its definition in mpmath: the log of the multivariate density over the
    product of its marginals, from the correlation matrix itself
  * the units of the two and the largest errors observed
  * the small problems of the GPU tests, and the tree of the sums"""
import math

import mpmath
import numpy as np
from scipy import special

from tests import box_prob_cases as bc
from tests import t_box_cases as tb
from tests import t_copula_cases as tc

U = 2.0 ** -53
MP_DIGITS = 40
DOFS = tc.DOFS

# the constants of copula_t.hip
T_NEWTON_CAP = 40
T_LOG_START = -0.7

# The largest errors observed against the references, in q_units / l_units: of the twins on this file's arguments (CPU test, printed
# with -s and asserted) and of the device (tests/test_gpu_copula_lik.py prints them).  The gates are twice the twins' figures.
Q_UNITS_OBSERVED_TWIN = 14.84    # nu = 64 at p = 0.9
L_UNITS_OBSERVED_TWIN = 1.99     # M = 64, nu = 1 (M64-G3-n200-coarse)
Q_UNITS_GATE = 2.0 * Q_UNITS_OBSERVED_TWIN
L_UNITS_GATE = 2.0 * L_UNITS_OBSERVED_TWIN
Q_UNITS_OBSERVED = 14.42         # MI355X: nu = 64 at p = 0.1; per nu 3.3, 3.0, 3.0, 2.1, 4.1, 4.8, 10.7, 14.4
L_UNITS_OBSERVED = 1.82          # MI355X: M = 128; per shape 0, 1.00, 1.41, 1.17, 1.80, 1.82


class Trips(tc.Trips):
    def __init__(self):
        super().__init__()
        self.t_newton = 0


# ---- the t quantile ----------------------------------------------------------------------------------------------------------

def twin_t_lower_root(C, p, trips):
    """t >= 0 with T_nu(-t) = p, 0 < p <= 1/2"""
    nu = C.dof
    lr = math.log(p * C.sqrt_dof / C.c0) / nu
    in_log = lr < T_LOG_START
    if in_log:
        try:
            t = C.sqrt_dof * math.exp(-lr)
        except OverflowError:
            return math.inf
        if t == math.inf:
            return t
    else:
        z = -float(special.ndtri(p))
        z2 = z * z
        t = z + z * (z2 + 1.0) / (4.0 * nu) + z * ((5.0 * z2 + 16.0) * z2 + 3.0) / (96.0 * nu * nu)
    done = False
    it = 0
    for it in range(T_NEWTON_CAP):
        T = tc.twin_t_lower(C, t, trips)
        if not T > 0.0:
            step = -3.0 if in_log else -0.5 * t
        else:
            rel = (T - p) / p
            g = math.log1p(rel) if abs(rel) < 0.5 else math.log(T / p)
            if t < C.sqrt_dof:
                h = C.c0 * math.exp(-C.A * math.log1p(t * t / nu)) / T
            else:
                r = C.sqrt_dof / t
                h = (C.c0 / C.sqrt_dof) * tc._pow(r, nu) * math.exp(-C.A * math.log1p(r * r)) / T * (nu / t)
            w = 2.0 * C.A / (nu / t + t)
            if in_log:
                th = t * h
                den = min(max(1.0 - 0.5 * g * (w / h - 1.0 - 1.0 / th), 0.5), 2.0)
                step = min(max(g / th / den, -3.0), 3.0)
            else:
                den = min(max(1.0 - 0.5 * g * (w / h - 1.0), 0.5), 2.0)
                step = min(max(g / h / den, -0.5 * t), max(1.0, t))
                if abs(step) <= 2.0 ** -30 * max(t, 1.0 / h):
                    t += step
                    done = True
                    break
        if in_log:
            t *= math.exp(step)
            if abs(step) <= 2.0 ** -30:
                done = True
                break
        else:
            t += step
    trips.note("t_newton", it + 1, T_NEWTON_CAP, done)
    return t


def twin_t_quantile(C, p, trips):
    if not 0.0 <= p <= 1.0:
        return math.nan
    if p == 0.0:
        return -math.inf
    if p == 1.0:
        return math.inf
    if p == 0.5:
        return 0.0
    return -twin_t_lower_root(C, p, trips) if p <= 0.5 else twin_t_lower_root(C, 1.0 - p, trips)


def p_arguments():
    """the probabilities of the accuracy tests: the levels of tests/t_box_cases.py, the clamps, two deep tails and the neighbours
    of 1/2"""
    extra = [U, 1.0 - U, 1e-30, 1e-300, float(np.nextafter(0.5, 0.0)), float(np.nextafter(0.5, 1.0))]
    return np.unique(np.concatenate([tb.LEVELS, extra]))


def mp_t_quantile(dof, p, start):
    """T_dof^-1 at the double p in (0, 1), as an mpf: the root of log T - log p in the lower tail (for p > 1/2 by symmetry; 1 - p
    is exact in the working precision), by the secant method from the double `start`"""
    p = float(p)
    if p == 0.5:
        return mpmath.mpf(0)
    with mpmath.workdps(MP_DIGITS):
        nu = mpmath.mpf(float(dof))
        pl = mpmath.mpf(p) if p < 0.5 else 1 - mpmath.mpf(p)
        logp = mpmath.log(pl)
        s = -abs(mpmath.mpf(float(start)))
        y = mpmath.findroot(lambda t: mpmath.log(tb._mp_t_lower(nu, t)) - logp, (s * (1 + mpmath.mpf(2) ** -40), s), solver="secant",
                            tol=mpmath.mpf(10) ** -(MP_DIGITS - 8), maxsteps=60)
        y = -abs(y)
        return y if p < 0.5 else -y


def q_units(y, ref, p, dof):
    """|y - ref| / (2^-53 max(|ref|, min(p, 1 - p) / t_nu(ref))): the second term is what a relative perturbation of p by one
    rounding moves the quantile by"""
    with mpmath.workdps(MP_DIGITS):
        nu = mpmath.mpf(float(dof))
        dens = mpmath.gamma((nu + 1) / 2) / (mpmath.sqrt(nu * mpmath.pi) * mpmath.gamma(nu / 2)) * (1 + ref * ref / nu) ** (-(nu + 1) / 2)
        pm = mpmath.mpf(float(p))
        scale = U * max(abs(ref), min(pm, 1 - pm) / dens)
        return float(abs(mpmath.mpf(float(y)) - ref) / scale)


# ---- the log density ----------------------------------------------------------------------------------------------------------

def model_constant(M, dof):
    """c_g of the header as the library forms it: in extended precision, rounded to a double; 0 for the Gaussian model and M = 1"""
    if dof == np.inf or M == 1:
        return 0.0
    with mpmath.workdps(30):
        nu = mpmath.mpf(float(dof))
        return float(mpmath.loggamma((nu + M) / 2) + (M - 1) * mpmath.loggamma(nu / 2) - M * mpmath.loggamma((nu + 1) / 2))


def inverse_factor(corr):
    """A [M, M] lower triangular with A corr A^T = 1, and logdet = sum log L_ii, from a correlation matrix"""
    L = np.linalg.cholesky(np.asarray(corr, dtype=np.float64))
    A = np.linalg.solve(L, np.eye(L.shape[0]))
    return np.ascontiguousarray(np.tril(A)), float(np.sum(np.log(np.diag(L))))


def twin_log_density(A, logdet, dof, y):
    """the chain of k_lik_chain in fp64 for scores y [M, n]: -> l [n]"""
    A = np.asarray(A, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    M, n = y.shape
    gauss = dof == np.inf
    cg = model_constant(M, dof)
    Q = np.zeros(n)
    P = np.zeros(n)
    with np.errstate(all="ignore"):
        for i in range(M):
            v = np.zeros(n)
            for k in range(i):
                v = v + A[i, k] * y[k]
            v = v + A[i, i] * y[i]
            Q = Q + v * v
            y2 = y[i] * y[i]
            P = P + (y2 if gauss else np.log1p(y2 / dof))
        if gauss:
            return -0.5 * (Q + -P) + -logdet
        return ((cg + -logdet) + -((0.5 * (dof + M)) * np.log1p(Q / dof))) + (0.5 * (dof + 1.0)) * P


def long_double_log_density(A, logdet, dof, y):
    """the formula of the header in long double from the fp64 A, logdet and scores y [M, n] -> (l [n] long double, scale [n] fp64);
    scale = the sum of the absolute values of every term the formula adds, plus the first-order effect of rounding the dot
    products, sum_i |dl / dv_i| sum_k |A_ik y_k|: l_units divides by 2^-53 of it"""
    ld = np.longdouble
    A = np.tril(np.asarray(A, dtype=np.float64)).astype(ld)
    y = np.asarray(y, dtype=np.float64).astype(ld)
    M, n = y.shape
    v = A @ y
    absdot = np.abs(A) @ np.abs(y)
    Q = np.sum(v * v, axis=0)
    if dof == np.inf:
        S = np.sum(y * y, axis=0)
        l = -(Q - S) / 2 - ld(logdet)
        scale = Q / 2 + S / 2 + abs(ld(logdet)) + np.sum(np.abs(v) * absdot, axis=0)
    else:
        nu = ld(dof)
        with mpmath.workdps(30):
            m = mpmath.mpf(float(dof))
            cg = ld(0) if M == 1 else ld(mpmath.nstr(mpmath.loggamma((m + M) / 2) + (M - 1) * mpmath.loggamma(m / 2)
                                                      - M * mpmath.loggamma((m + 1) / 2), 25))
        P = np.sum(np.log1p(y * y / nu), axis=0)
        t1, t2 = (nu + M) / 2 * np.log1p(Q / nu), (nu + 1) / 2 * P
        l = cg - ld(logdet) - t1 + t2
        scale = abs(cg) + abs(ld(logdet)) + t1 + t2 + np.sum((nu + M) * np.abs(v) / (nu + Q) * absdot, axis=0)
    return l, scale.astype(np.float64)


def l_units(l, ref, scale):
    """|l - ref| / (2^-53 scale), ref and scale from long_double_log_density (0 where the scale is 0 and the two agree)"""
    err = np.abs(np.asarray(l, dtype=np.float64).astype(np.longdouble) - ref).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.where(scale > 0.0, err / (U * scale), np.where(err == 0.0, 0.0, np.inf))


def mp_log_density(A, dof, y):
    """the definition, for one column of scores y [M]: log of the multivariate normal / t density with the correlation matrix
    R = (A^T A)^-1 of the fp64 A, over the product of its marginals, in mpmath from R itself (its determinant and inverse)"""
    with mpmath.workdps(MP_DIGITS):
        M = len(y)
        Am = mpmath.matrix([[mpmath.mpf(float(A[i][k])) if k <= i else mpmath.mpf(0) for k in range(M)] for i in range(M)])
        R = mpmath.inverse(Am.T * Am)
        ym = mpmath.matrix([mpmath.mpf(float(v)) for v in y])
        quad = (ym.T * mpmath.inverse(R) * ym)[0]
        logdet_r = mpmath.log(mpmath.det(R))
        if dof == np.inf:
            joint = -quad / 2 - logdet_r / 2 - M * mpmath.log(2 * mpmath.pi) / 2
            marg = sum(-v * v / 2 - mpmath.log(2 * mpmath.pi) / 2 for v in ym)
        else:
            nu = mpmath.mpf(float(dof))
            joint = (mpmath.loggamma((nu + M) / 2) - mpmath.loggamma(nu / 2) - M * mpmath.log(nu * mpmath.pi) / 2 - logdet_r / 2
                     - (nu + M) / 2 * mpmath.log1p(quad / nu))
            marg = sum(mpmath.loggamma((nu + 1) / 2) - mpmath.loggamma(nu / 2) - mpmath.log(nu * mpmath.pi) / 2
                       - (nu + 1) / 2 * mpmath.log1p(v * v / nu) for v in ym)
        return joint - marg


# ---- the problems of the tests -------------------------------------------------------------------------------------------------

SHAPES = ((1, 1, 1, False), (2, 3, 63, True), (3, 16, 64, True), (17, 2, 65, False), (64, 3, 200, True), (128, 2, 130, True))
MODEL_DOFS = (np.inf, 3.0, 1.0, 64.0, 4.5, 8.0, np.inf, 2.0, 30.0, 1.5, 5.0, 6.0, 10.0, 15.0, 20.0, 2.5)


def correlation(M, g, seed=0):
    """model g's correlation matrix: equicorrelation 0.9 for g = 1, else that of a random factor"""
    if g == 1:
        c = np.full((M, M), 0.9)
        np.fill_diagonal(c, 1.0)
        return c
    F = bc.chol_factor(M, 1000 * seed + 17 * g + M)
    c = F @ F.T
    c = 0.5 * (c + c.T)
    np.fill_diagonal(c, 1.0)
    return c


class Problem:
    """(M, G, n, coarse): the models (A [G, M, M], logdet [G], dofs [G]) and the uniforms [M, ld] with ld > n: NaN at columns 0, 63,
    64 and the last (fine only, coarse only, alternating), and u at 0, 1, 2^-53 and 1 - 2^-53 in kept columns"""

    def __init__(self, M, G, n, coarse, seed=0):
        self.M, self.G, self.n, self.ld = M, G, n, n + 5
        self.dofs = np.array(MODEL_DOFS[:G], dtype=np.float64)
        fac = [inverse_factor(np.ones((1, 1)) if M == 1 else correlation(M, g, seed)) for g in range(G)]
        self.A = np.ascontiguousarray(np.stack([f[0] for f in fac]))
        self.logdet = np.array([f[1] for f in fac])
        rng = np.random.default_rng([seed, M, G, n])
        self.u_fine = self._uniforms(rng)
        self.u_coarse = self._uniforms(rng, like=self.u_fine) if coarse else None
        # u at 0, 1 and the two clamps in kept columns 1 .. 8, alternating between the sides
        for j, c in enumerate(range(1, min(n - 1, 9))):
            side = self.u_coarse if (coarse and j % 2) else self.u_fine
            side[(3 * j) % M, c] = (0.0, 1.0, U, 1.0 - U)[(j // 2) % 4 if coarse else j % 4]
        # NaN at columns 0, 63, 64 and the last: in fine only and in coarse only, alternating
        self.dropped = [c for c in sorted({0, 63, 64, n - 1}) if c < n] if n > 1 else []
        for j, c in enumerate(self.dropped):
            side = self.u_coarse if (coarse and j % 2) else self.u_fine
            side[(5 * j) % M, c] = np.nan
        self.keep = np.ones(n, dtype=bool)
        self.keep[self.dropped] = False

    def _uniforms(self, rng, like=None):
        u = np.full((self.M, self.ld), 0.25)           # the padding beyond n is not read
        z = rng.standard_normal((self.M, self.n))
        if like is not None:
            z = 0.9 * special.ndtri(np.clip(like[:, :self.n], 1e-12, 1 - 1e-12)) + math.sqrt(1.0 - 0.81) * z
        u[:, :self.n] = special.ndtr(1.5 * z)
        return u

    def __repr__(self):
        return "M{}-G{}-n{}{}".format(self.M, self.G, self.n, "-coarse" if self.u_coarse is not None else "")


def clamp(u):
    return np.minimum(np.maximum(u, U), 1.0 - U)


def tree_sums(ll_fine, ll_coarse):
    """the sums of the header from the returned columns ll_fine, ll_coarse [G, n] (coarse None: 0), NaN in dropped columns:
    -> (kept, sums [3 G + G G]) by the documented tree (tests/box_prob_cases.tree_sum from column 0)"""
    G, n = ll_fine.shape
    keep = ~np.isnan(ll_fine[0])
    lf = np.where(keep, ll_fine, 0.0)
    lc = np.zeros_like(lf) if ll_coarse is None else np.where(keep, ll_coarse, 0.0)
    d = np.where(keep, lf - lc, 0.0)
    out = [bc.tree_sum(lf[g], 0) for g in range(G)] + [bc.tree_sum(lc[g], 0) for g in range(G)] + [bc.tree_sum(d[g], 0) for g in range(G)]
    out += [bc.tree_sum(d[g] * d[h], 0) for g in range(G) for h in range(G)]
    return int(np.count_nonzero(keep)), np.array(out)
