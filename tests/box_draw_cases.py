"""The draws of mlmc_copula_box_draws_batch (include/mlmc_hip.h: the chain of the box probabilities with a draw of every component,
the GHK sampler) restated on the host, shared by tests/test_box_draws_cpu.py and tests/test_gpu_box_draws.py.  Nothing here
touches the device.  The points, the problems, the summation tree and the closed-form constants are those of
tests/box_prob_cases.py.

  twin       the header's chain operation by operation in NumPy fp64 with scipy.special.ndtr / ndtri: weights, z and u;
  reference  the same chain on the same points in mpmath (MP_DIGITS digits).

The unit of an error of z_i at a point is 2^-53 x a CONDITION SCALE E_z that the twin carries along: the recursion at the top of
box_prob_cases.py (E_s, E_d, E_width, E_p, E_y, now for every i) and, for z_i = s + L_ii y_i,
    E_z = E_s + |L_ii| E_y + 2 |L_ii y_i| + |z_i|
(the errors of s and y, the roundings of the product and of the sum)."""
import functools

import mpmath
import numpy as np
from scipy import special, stats

from tests import joint_sample_cases as jc
from tests.box_prob_cases import (CLOSED_N, CORR3, DEVICE_MARGIN, MAX_M, MP_DIGITS, P_HI, P_LO, RHO2, SEEDS8, U, Case, _mp_ndtri, _phi,  # noqa: F401
                                  boxes, chol_factor, points, tree_mean)

U_LO, U_HI = jc.U_LO, jc.U_HI

# The twin's largest error of z against the reference over POINT_CASES, in the unit above, as tests/test_box_draws_cpu.py measures
# it (it prints the figure and fails if it is larger than this record).
TWIN_Z_UNITS_OBSERVED = 0.92       # M3-cond, component 0 of a lower half-space: SciPy's ndtri, which is not correctly rounded
# the allowance box_prob_cases derives for the device's normcdf / normcdfinv
GPU_Z_TOLERANCE_UNITS = TWIN_Z_UNITS_OBSERVED * DEVICE_MARGIN


def twin(L, lo, hi, shift, w):
    """(f [n], z [M, n], u [M, n], e_z [M, n]) of one box on the points w [M, n]: weights, scores, their clamped Phi and the
    condition scale of z"""
    L = np.asarray(L, dtype=np.float64)
    M = L.shape[0]
    n = w.shape[1]
    f = np.ones(n)
    y, e_y = np.zeros((M, n)), np.zeros((M, n))
    z, e_z = np.zeros((M, n)), np.zeros((M, n))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(M):
            s = np.full(n, 0.0 if shift is None else float(shift[i]))
            mag, e_s = np.zeros(n), np.zeros(n)
            for k in range(i):
                t = L[i, k] * y[k]
                s = s + t
                mag += np.abs(t)
                e_s += abs(L[i, k]) * e_y[k]
            e_s += (i + 1) * mag + i * (0.0 if shift is None else abs(float(shift[i])))
            a, b = (lo[i] - s) / L[i, i], (hi[i] - s) / L[i, i]
            refl = a > 0.0
            xd, xe = np.where(refl, -b, a), np.where(refl, -a, b)
            d, e = special.ndtr(xd), special.ndtr(xe)
            width = e - d if lo[i] < hi[i] else np.zeros(n)
            f = f * width
            e_d = _phi(xd) * np.where(np.isfinite(xd), e_s / L[i, i] + 2 * np.abs(xd), 0.0) + d
            e_e = _phi(xe) * np.where(np.isfinite(xe), e_s / L[i, i] + 2 * np.abs(xe), 0.0) + e
            e_w = e_d + e_e + width
            p = np.minimum(np.maximum(d + w[i] * width, P_LO), P_HI)
            yy = special.ndtri(p)
            y[i] = np.where(refl, -yy, yy)
            e_y[i] = (e_d + w[i] * e_w + 2 * p) / np.maximum(_phi(yy), 1e-300) + np.abs(yy)
            t = L[i, i] * y[i]
            z[i] = np.minimum(np.maximum(s + t, lo[i]), hi[i])
            e_z[i] = e_s + abs(L[i, i]) * e_y[i] + 2 * np.abs(t) + np.abs(z[i])
    u = np.minimum(np.maximum(special.ndtr(z), U_LO), U_HI)
    return f, z, u, e_z


def reference(L, lo, hi, shift, w):
    """z at every point as a list [n] of lists [M] of mpf: the chain of the header in MP_DIGITS digits"""
    L = np.asarray(L, dtype=np.float64)
    M = L.shape[0]
    out = []
    with mpmath.workdps(MP_DIGITS):
        inf = mpmath.inf
        mp = lambda v: mpmath.mpf(float(v)) if np.isfinite(v) else (inf if v > 0 else -inf)       # noqa: E731
        Lm = [[mpmath.mpf(float(L[i, k])) for k in range(i + 1)] for i in range(M)]
        lom, him = [mp(v) for v in lo], [mp(v) for v in hi]
        shm = [mpmath.mpf(0) if shift is None else mpmath.mpf(float(shift[i])) for i in range(M)]
        p_lo, p_hi = mpmath.mpf(P_LO), mpmath.mpf(P_HI)
        for c in range(w.shape[1]):
            y, z = [], []
            for i in range(M):
                s = shm[i] + sum((Lm[i][k] * y[k] for k in range(i)), mpmath.mpf(0))
                a, b = (lom[i] - s) / Lm[i][i], (him[i] - s) / Lm[i][i]
                refl = a > 0
                d, e = (mpmath.ncdf(-b), mpmath.ncdf(-a)) if refl else (mpmath.ncdf(a), mpmath.ncdf(b))
                width = e - d if lo[i] < hi[i] else mpmath.mpf(0)
                yy = _mp_ndtri(min(max(d + mpmath.mpf(float(w[i, c])) * width, p_lo), p_hi))
                y.append(-yy if refl else yy)
                z.append(min(max(s + Lm[i][i] * y[i], lom[i]), him[i]))
            out.append(z)
    return out


def z_units(z, ref, e_z):
    """|z - ref| in the unit of this file for z [M, n], ref [n][M] of mpf, e_z [M, n]"""
    M, n = z.shape
    with mpmath.workdps(MP_DIGITS):
        return np.array([[float(abs(mpmath.mpf(float(z[i, c])) - ref[c][i]) / (U * float(e_z[i, c]))) for c in range(n)] for i in range(M)])


def draw_case(name, M, B, seeds, n, first, qmc, conditional=False, streams=None):
    """a Case of box_prob_cases (the same factor, boxes and shift) with M coordinates: the last draws the last component"""
    case = Case(name, M, B, seeds, n, first, qmc, conditional=conditional, streams=streams)
    case.coords = list(range(M)) if streams is None else list(streams)
    assert len(case.coords) == M
    return case


# against the extended reference, point by point: the point cases of box_prob_cases with one more coordinate
POINT_CASES = (
    draw_case("M1", 1, 3, (5,), 3, 0, True),
    draw_case("M2-sobol", 2, 4, (0, 9), 65, 0, True),
    draw_case("M2-philox", 2, 4, (3,), 65, 777, False),
    draw_case("M3-cond", 3, 4, (1,), 64, 4096, True, conditional=True),
    draw_case("M5-philox-cond", 5, 3, (2,), 63, 0, False, conditional=True, streams=(9, 4, 4, 70000, 11)),
    draw_case("M17", 17, 2, (4,), 33, 4095, True, streams=tuple(range(1007, 1024))),
    draw_case("M64", 64, 1, (6,), 17, 0, True),
    draw_case("M128-cap", MAX_M, 1, (8,), 5, 62, True),
)

# equality with the box-probability entry and the bounds: n = 1, 63, 64, 65, 1000 at aligned and odd first, M = 1 .. 128, B up to 37,
# R up to 8, with and without shift, Sobol' and Philox
SHAPE_CASES = (
    draw_case("n1", 3, 1, (0,), 1, 0, True),
    draw_case("n63", 5, 3, (0,), 63, 0, True),
    draw_case("n64", 2, 1, SEEDS8, 64, 4096, True),
    draw_case("n65-philox", 3, 3, (1,), 65, 777, False),
    draw_case("n1000", 5, 37, (2,), 1000, 4096, True),
    draw_case("M1-n64", 1, 5, (3, 4), 64, 0, True, conditional=True),
    draw_case("M17-n1000-cond", 17, 3, (3,), 1000, 777, True, conditional=True),
    draw_case("M64-n65", 64, 3, (7,), 65, 0, False),
    draw_case("cap-n64", MAX_M, 1, (1,), 64, 64, True),
)


@functools.lru_cache(maxsize=None)
def case_twin(case):
    """(f [R, B, n], z [R, B, M, n], u [R, B, M, n], e_z [R, B, M, n]) of the twin"""
    R = len(case.seeds)
    f = np.empty((R, case.B, case.n))
    z = np.empty((R, case.B, case.M, case.n))
    u, k = np.empty_like(z), np.empty_like(z)
    for r, seed in enumerate(case.seeds):
        w = case.w(seed)
        for b in range(case.B):
            f[r, b], z[r, b], u[r, b], k[r, b] = twin(case.L, case.lo[b], case.hi[b], None if case.shift is None else case.shift[b], w)
    for v in (f, z, u, k):
        v.setflags(write=False)
    return f, z, u, k


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """the reference z of every (seed, box): a list [R][B] of lists [n][M] of mpf"""
    return [[reference(case.L, case.lo[b], case.hi[b], None if case.shift is None else case.shift[b], case.w(seed))
             for b in range(case.B)] for seed in case.seeds]


def worst_z_units(z, case):
    """the largest error of z [R, B, M, n] against the reference of a point case, in the twin's unit"""
    e_z = case_twin(case)[3]
    ref = case_reference(case)
    return max(float(z_units(z[r, b], ref[r][b], e_z[r, b]).max()) for r in range(len(case.seeds)) for b in range(case.B))


# ---- closed forms: conditional means of a bivariate normal ------------------------------------------------------------------------
L2 = np.linalg.cholesky(np.array([[1.0, RHO2], [RHO2, 1.0]]))
CLOSED_LIMITS = ((0.0, 0.0), (1.5, -0.5), (2.5, 2.0))            # (h, k): the event Z_0 > h, Z_1 > k


def orthant_probability(h, k, rho=RHO2):
    """P(Z_0 > h, Z_1 > k) = P(-Z_0 < -h, -Z_1 < -k); at (0, 0) the closed form 1/4 + asin(rho) / 2 pi"""
    if h == 0.0 and k == 0.0:
        return 0.25 + np.arcsin(rho) / (2 * np.pi)
    return float(stats.multivariate_normal([0.0, 0.0], [[1.0, rho], [rho, 1.0]]).cdf([-h, -k]))


def conditional_mean_z0(h, k, rho=RHO2):
    """E[Z_0 | Z_0 > h, Z_1 > k] (Rosenbaum 1961)"""
    c = np.sqrt(1.0 - rho * rho)
    phi = lambda x: np.exp(-0.5 * x * x) / np.sqrt(2 * np.pi)       # noqa: E731
    num = phi(h) * (1.0 - special.ndtr((k - rho * h) / c)) + rho * phi(k) * (1.0 - special.ndtr((h - rho * k) / c))
    return float(num / orthant_probability(h, k, rho))


HALF_SPACE = 2.0                                                   # the event Z_0 > 2 alone


def half_space_means(rho=RHO2):
    """(E[Z_0 | Z_0 > 2], E[Z_1 | Z_0 > 2])"""
    m = float(np.exp(-0.5 * HALF_SPACE ** 2) / np.sqrt(2 * np.pi) / special.ndtr(-HALF_SPACE))
    return m, rho * m


def closed_form_events():
    """(name, lo [2], hi [2], component, exact)"""
    inf = np.full(2, np.inf)
    out = [("h{}k{}".format(h, k), np.array([h, k]), inf, 0, conditional_mean_z0(h, k)) for h, k in CLOSED_LIMITS]
    m0, m1 = half_space_means()
    out += [("half-z0", np.array([HALF_SPACE, -np.inf]), inf, 0, m0), ("half-z1", np.array([HALF_SPACE, -np.inf]), inf, 1, m1)]
    return out


def ratio_summary(f, x):
    """(mean, stderr) of the seeds' ratios sum f x / sum f for f [R, n], x [R, n]"""
    r = (f * x).sum(axis=1) / f.sum(axis=1)
    return r.mean(), np.std(r, ddof=1) / np.sqrt(r.size)


def ess(f):
    """(sum f)^2 / sum f^2 over the last axis; NaN where every weight is 0"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return f.sum(axis=-1) ** 2 / (f * f).sum(axis=-1)
