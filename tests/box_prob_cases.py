"""The integrand of mlmc_copula_box_prob_batch (include/mlmc_hip.h; Genz's separation of variables) restated on the host, shared by
tests/test_box_prob_cpu.py and tests/test_gpu_box_prob.py.  Nothing here touches the device.

  twin       the header's chain operation by operation in NumPy fp64 with scipy.special.ndtr / ndtri, vectorised over the points;
  reference  the same chain on the same points in mpmath (MP_DIGITS digits; Phi^-1 by two Newton steps from ndtri);
  tree_mean  the header's summation tree;
  points     the coordinates w_i: `sobol_table` of the package (host arithmetic) or the NumPy Philox of tests/sample_cases.py.

The unit of an error of f at a point is 2^-53 x the point's CONDITION SCALE x f.  The scale is a first-order bound of the relative
error of f in units of 2^-53 if every fp64 operation and every Phi / Phi^-1 were rounded correctly, carried along the chain by the
twin (E_x = absolute error of x in units of 2^-53, phi = the normal density):
    E_s  = sum_k |L_ik| E_y_k + (i + 1) sum_k |L_ik y_k| + i |shift_i|
    E_a' = E_s / L_ii + 2 |a'|   (0 for an infinite limit; likewise b')
    E_d  = phi(a') E_a' + d,  E_e likewise;   E_width = E_d + E_e + width;   scale += E_width / width + 1
    E_p  = E_d + w E_width + 2 p;   E_y = E_p / phi(y) + |y|
A device whose Phi and Phi^-1 err by k ulp stays within about k units."""
import functools

import mpmath
import numpy as np
from scipy import special

from tests import sample_cases as sc
from tests import sobol_cases as sb

U = 2.0 ** -53
MP_DIGITS = 40
P_LO, P_HI = 2.0 ** -1022, 1.0 - 2.0 ** -53
MAX_M = 128                                            # MLMC_BOX_PROB_MAX_M

# The twin's largest error against the reference over POINT_CASES, in the unit above, as tests/test_box_prob_cpu.py measures it
# (it prints the figure and fails if it is larger than this record).
TWIN_UNITS_OBSERVED = 0.45
# The device's normcdf / normcdfinv are not correctly rounded: tests/joint_sample_cases.py records 3.2 and 3.4 ulp on an MI355X and
# allows 16 (4 x, rounded up to a power of two).  The scale counts one ulp per evaluation and the twin, with SciPy's functions, stays
# below one unit, so the device may take 16 times the twin's figure.
DEVICE_MARGIN = 16.0
GPU_TOLERANCE_UNITS = TWIN_UNITS_OBSERVED * DEVICE_MARGIN          # 7.2; tests/test_gpu_box_prob.py prints what an MI355X takes: 0.34

SEEDS8 = tuple(range(8))
# Phi(-6) through exp(-x^2 / 2): the argument 18 carries up to 2 roundings of 18 ulp each, the rest of the evaluation the margin
TAIL6_BOUND = (2 * 18 + DEVICE_MARGIN) * 2 * U


def points(seed, coords, first, n, qmc):
    """w [len(coords), n]: coordinate coords[i] of the points first .. first + n - 1 under `seed`"""
    if len(coords) == 0:
        return np.zeros((0, n))
    idx = np.uint64(first) + np.arange(n, dtype=np.uint64)
    if not qmc:
        return np.array([sc.stream_uniforms(seed, s, idx) for s in coords]).reshape(len(coords), n)
    from mlmc_amd.tool.simple_distribution import sobol_table
    dirs, shift = sobol_table(seed, np.asarray(coords, dtype=np.int64))
    return sb.to_unit(sb.raw_points(dirs, idx) ^ shift[:, None])


def _phi(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(np.isfinite(x), np.exp(-0.5 * x * x) / np.sqrt(2 * np.pi), 0.0)


def twin(L, lo, hi, shift, w, reflect=True):
    """(f [n], scale [n]) of one box on the points w [M - 1, n]"""
    L = np.asarray(L, dtype=np.float64)
    M = L.shape[0]
    n = w.shape[1] if M > 1 else max(w.shape[1], 1)
    f, scale = np.ones(n), np.zeros(n)
    y, e_y = np.zeros((max(M - 1, 0), n)), np.zeros((max(M - 1, 0), n))
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
            refl = (a > 0.0) if reflect else np.zeros(n, dtype=bool)
            xd, xe = np.where(refl, -b, a), np.where(refl, -a, b)
            d, e = special.ndtr(xd), special.ndtr(xe)
            width = e - d if lo[i] < hi[i] else np.zeros(n)
            f = f * width
            e_d = _phi(xd) * np.where(np.isfinite(xd), e_s / L[i, i] + 2 * np.abs(xd), 0.0) + d
            e_e = _phi(xe) * np.where(np.isfinite(xe), e_s / L[i, i] + 2 * np.abs(xe), 0.0) + e
            e_w = e_d + e_e + width
            scale += np.where(width > 0, e_w / np.where(width > 0, width, 1.0), 0.0) + 1.0
            if i < M - 1:
                p = np.minimum(np.maximum(d + w[i] * width, P_LO), P_HI)
                yy = special.ndtri(p)
                y[i] = np.where(refl, -yy, yy)
                e_y[i] = (e_d + w[i] * e_w + 2 * p) / np.maximum(_phi(yy), 1e-300) + np.abs(yy)
    return f, scale


def _mp_ndtri(p):
    y = mpmath.mpf(float(special.ndtri(float(p))))
    for _ in range(2):
        y = y - (mpmath.ncdf(y) - p) / mpmath.npdf(y)
    return y


def reference(L, lo, hi, shift, w):
    """f at every point as a list of mpf: the chain of the header in MP_DIGITS digits"""
    L = np.asarray(L, dtype=np.float64)
    M = L.shape[0]
    n = w.shape[1] if M > 1 else max(w.shape[1], 1)
    out = []
    with mpmath.workdps(MP_DIGITS):
        inf = mpmath.inf
        mp = lambda v: mpmath.mpf(float(v)) if np.isfinite(v) else (inf if v > 0 else -inf)       # noqa: E731
        Lm = [[mpmath.mpf(float(L[i, k])) for k in range(i + 1)] for i in range(M)]
        lom, him = [mp(v) for v in lo], [mp(v) for v in hi]
        shm = [mpmath.mpf(0) if shift is None else mpmath.mpf(float(v)) for v in (lo if shift is None else shift)]
        p_lo, p_hi = mpmath.mpf(P_LO), mpmath.mpf(P_HI)
        for c in range(n):
            f, y = mpmath.mpf(1), []
            for i in range(M):
                s = shm[i] + sum((Lm[i][k] * y[k] for k in range(i)), mpmath.mpf(0))
                a, b = (lom[i] - s) / Lm[i][i], (him[i] - s) / Lm[i][i]
                refl = a > 0
                d, e = (mpmath.ncdf(-b), mpmath.ncdf(-a)) if refl else (mpmath.ncdf(a), mpmath.ncdf(b))
                width = e - d if lo[i] < hi[i] else mpmath.mpf(0)
                f *= width
                if i < M - 1:
                    yy = _mp_ndtri(min(max(d + mpmath.mpf(float(w[i, c])) * width, p_lo), p_hi))
                    y.append(-yy if refl else yy)
            out.append(f)
    return out


def units(f, ref, scale):
    """|f - ref| in the unit of this file, ref a list of mpf"""
    with mpmath.workdps(MP_DIGITS):
        tiny = mpmath.mpf(2.0 ** -1022)
        return np.array([float(abs(mpmath.mpf(float(a)) - r) / (U * float(k) * max(r, tiny))) for a, r, k in zip(np.ravel(f), ref, np.ravel(scale))])


def tree_sum(f, first):
    """the header's tree over the values f of the points first .. first + len(f) - 1"""
    f = np.asarray(f, dtype=np.float64)
    n = f.size
    blk0 = first >> 6
    blocks = ((first + n - 1) >> 6) - blk0 + 1
    v = np.zeros(blocks * 64)
    v[first - 64 * blk0:first - 64 * blk0 + n] = f
    v = v.reshape(blocks, 64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v[:, :o] + v[:, o:2 * o]
    p = v[:, 0]
    acc = np.zeros(256)
    for k0 in range(0, blocks, 256):
        part = p[k0:k0 + 256]
        acc[:part.size] = acc[:part.size] + part
    for o in (128, 64, 32, 16, 8, 4, 2, 1):
        acc = acc[:o] + acc[o:2 * o]
    return acc[0]


def tree_mean(f, first, M=2):
    f = np.asarray(f, dtype=np.float64)
    return f[0] if M == 1 else tree_sum(f, first) / float(f.size)


# ---- the problems ---------------------------------------------------------------------------------------------------------------
def chol_factor(M, seed):
    """the unit-row lower Cholesky factor of a random correlation matrix (of 4 M + 3 samples: its diagonal stays near 0.85)"""
    a = np.random.default_rng(seed).standard_normal((M, 4 * M + 3))
    c = a @ a.T
    d = 1.0 / np.sqrt(np.diag(c))
    c = c * d[:, None] * d[None, :]
    low = np.linalg.cholesky(0.5 * (c + c.T))
    return np.ascontiguousarray(low / np.sqrt(np.sum(low * low, axis=1))[:, None])


def equicorrelation_factor(M, rho=0.5):
    c = np.full((M, M), rho)
    np.fill_diagonal(c, 1.0)
    return np.linalg.cholesky(c)


def boxes(M, B, seed):
    """B boxes [B, M] in score space that cycle through: a central box, an upper-tail orthant-like box, a lower half-space in
    every component, a far box in component 0"""
    rng = np.random.default_rng(seed)
    lo, hi = np.empty((B, M)), np.empty((B, M))
    for b in range(B):
        kind = b % 4
        if kind == 0:
            lo[b], hi[b] = -rng.uniform(0.5, 2.0, M), rng.uniform(0.5, 2.0, M)
        elif kind == 1:
            lo[b], hi[b] = rng.uniform(-1.0, 1.0, M), np.inf
            lo[b, 0] = 1.5
        elif kind == 2:
            lo[b], hi[b] = -np.inf, rng.uniform(0.0, 2.0, M)
        else:
            lo[b], hi[b] = -rng.uniform(1.0, 3.0, M), rng.uniform(1.0, 3.0, M)
            lo[b, 0], hi[b, 0] = 2.0, 3.0
    return lo, hi


class Case:
    def __init__(self, name, M, B, seeds, n, first, qmc, conditional=False, streams=None):
        self.name, self.M, self.B, self.seeds, self.n, self.first, self.qmc = name, M, B, tuple(seeds), n, first, qmc
        self.L = chol_factor(M, 100 + M)
        self.shift = None
        if conditional:                                # rows that are not of unit norm, and a mean per box
            rng = np.random.default_rng(7 * M)
            self.L = self.L * rng.uniform(0.3, 1.0, M)[:, None]
            self.shift = rng.uniform(-1.0, 1.0, (B, M))
        self.lo, self.hi = boxes(M, B, 200 + M)
        self.streams = streams
        self.coords = list(range(M - 1)) if streams is None else list(streams)

    def __repr__(self):
        return self.name

    def w(self, seed):
        return points(seed, self.coords, self.first, self.n, self.qmc)


# against the extended reference, point by point (the reference costs about 0.3 ms per point and component)
POINT_CASES = (
    Case("M1", 1, 3, (5,), 3, 0, True),
    Case("M2-sobol", 2, 4, (0, 9), 65, 0, True),
    Case("M2-philox", 2, 4, (3,), 65, 777, False),
    Case("M3-cond", 3, 4, (1,), 64, 4096, True, conditional=True),
    Case("M5-philox-cond", 5, 3, (2,), 63, 0, False, conditional=True, streams=(9, 4, 4, 70000)),
    Case("M17", 17, 2, (4,), 33, 4095, True, streams=tuple(range(1007, 1023))),
    Case("M64", 64, 1, (6,), 17, 0, True),
    Case("M128-cap", MAX_M, 1, (8,), 5, 62, True),
)

# against the twin: the shapes (n, B, R, first and both kinds of points)
SHAPE_CASES = (
    Case("n1", 3, 1, (0,), 1, 0, True),
    Case("n63", 5, 3, (0,), 63, 0, True),
    Case("n64", 2, 1, SEEDS8, 64, 4096, True),
    Case("n65-philox", 3, 3, (1,), 65, 777, False),
    Case("n1000", 5, 37, (2,), 1000, 4096, True),
    Case("n4096", 3, 3, SEEDS8, 4096, 0, True, conditional=True),
    Case("n4096-philox", 2, 37, SEEDS8, 4096, 12345, False),
    Case("M17-n1000", 17, 3, (3,), 1000, 777, True),
    Case("M64-n65", 64, 3, (7,), 65, 0, False),
    Case("cap-n64", MAX_M, 1, (1,), 64, 64, True),
)


@functools.lru_cache(maxsize=None)
def case_twin(case):
    """(f [R, B, n], scale [R, B, n]) of the twin"""
    f = np.empty((len(case.seeds), case.B, case.n))
    k = np.empty_like(f)
    for r, seed in enumerate(case.seeds):
        w = case.w(seed)
        for b in range(case.B):
            f[r, b], k[r, b] = twin(case.L, case.lo[b], case.hi[b], None if case.shift is None else case.shift[b], w)
    f.setflags(write=False)
    k.setflags(write=False)
    return f, k


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """the reference of every (seed, box): a list [R][B] of lists of mpf"""
    return [[reference(case.L, case.lo[b], case.hi[b], None if case.shift is None else case.shift[b], case.w(seed))
             for b in range(case.B)] for seed in case.seeds]


def reference_mean(ref):
    with mpmath.workdps(MP_DIGITS):
        return mpmath.fsum(ref) / len(ref)


# ---- closed forms ---------------------------------------------------------------------------------------------------------------
CLOSED_N = 4096
RHO2 = 0.6
CORR3 = np.array([[1.0, 0.5, -0.3], [0.5, 1.0, 0.2], [-0.3, 0.2, 1.0]])


def closed_forms():
    """(name, L, lo [M], hi [M], exact): orthant probabilities P(Y_m < 0 for all m)"""
    out = [("M2", np.linalg.cholesky(np.array([[1.0, RHO2], [RHO2, 1.0]])), 0.25 + np.arcsin(RHO2) / (2 * np.pi)),
           ("M3", np.linalg.cholesky(CORR3),
            0.125 + (np.arcsin(CORR3[0, 1]) + np.arcsin(CORR3[0, 2]) + np.arcsin(CORR3[1, 2])) / (4 * np.pi))]
    out += [("equi{}".format(M), equicorrelation_factor(M), 1.0 / (M + 1)) for M in (8, 16, 64)]
    return [(name, L, np.full(L.shape[0], -np.inf), np.zeros(L.shape[0]), exact) for name, L, exact in out]


def summary(replicates):
    """(prob, stderr) of the seeds' means [R]"""
    r = np.asarray(replicates)
    return r.mean(), np.std(r, ddof=1) / np.sqrt(r.size)
