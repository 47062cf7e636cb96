"""Genz's variable reordering (mlmc_copula_box_order_batch, include/mlmc_hip.h) restated on the host, shared by
tests/test_box_order_cpu.py, tests/test_gpu_box_order.py and tests/test_gpu_box_order_api.py.  Nothing here touches the device.

  order_twin  the header's algorithm operation by operation in NumPy, vectorised over the boxes and the components: fp64 with
              scipy.special.ndtr, or (real=np.longdouble) the same operations in long double with Phi from mpmath;
  margins     per box and step (second smallest w - smallest w) / smallest w: a permutation is compared with the device's only
              where every step of the box has a margin of at least MARGIN (the device's normcdf and exp are not scipy's);
  chain_stats the probability and its standard error over seeds from the chain twin of tests/box_prob_cases.py.

Given the permutation the factor does not depend on the widths: L is the plain Cholesky factor of the permuted covariance in a fixed
operation order, every operation one correctly rounded fp64 operation.  The unit of an error of an entry L_ji is 2^-53 x its
CONDITION SCALE (|C_cj| + sum_k |L_jk L_ck|) / L_ii, for the diagonal (C_jj + sum_k L_jk^2) / L_ii: what one rounding of the largest
term moves the entry by."""
import functools

import mpmath
import numpy as np
from scipy import special

from tests import box_prob_cases as bp

U = 2.0 ** -53
MARGIN = 1e-6
INV_SQRT_2PI = 0.3989422804014327
# the twin's largest error of an entry of L against its long-double version over the cases of tests/test_box_order_cpu.py, in the
# unit above, as that test measures it (it prints the figure and fails if it is larger than this record)
TWIN_UNITS_OBSERVED = 4.1                              # 4.03 measured, rounded up
GPU_TOLERANCE_UNITS = TWIN_UNITS_OBSERVED * bp.DEVICE_MARGIN


def _cdf(x, real):
    if real is np.float64:
        return special.ndtr(x)
    with mpmath.workdps(30):                           # long double: Phi in 30 digits, rounded to the 64-bit significand
        flat = [np.longdouble(mpmath.nstr(mpmath.ncdf(mpmath.mpf(repr(float(v))) if np.isfinite(v) else
                                                       (mpmath.inf if v > 0 else -mpmath.inf)), 25)) for v in np.ravel(x)]
    return np.array(flat, dtype=np.longdouble).reshape(np.shape(x))


def _pdf(x, real):
    return np.exp(real(-0.5) * (x * x)) * real(INV_SQRT_2PI)


class OrderResult:
    """perm [B, M]; L [B, M, M] the factor of the permuted covariance; ok [B]; margin [B, M]; scale [B, M, M] of the entries of L;
    y [B, M] the expected conditioned normals"""

    def __init__(self, perm, L, ok, margin, scale, y):
        self.perm, self.L, self.ok, self.margin, self.scale, self.y = perm, L, ok, margin, scale, y

    def qualifies(self):
        """[B]: every step of the box has a margin of at least MARGIN"""
        return np.all(self.margin >= MARGIN, axis=1)


def order_twin(C, lo, hi, shift=None, first=None, real=np.float64, forced_perm=None):
    """the header's algorithm for B boxes; C [M, M] or [B, M, M]; forced_perm [B, M]: take these components instead of the smallest
    widths (the long-double version follows the fp64 permutation)"""
    lo, hi = np.atleast_2d(np.asarray(lo, dtype=np.float64)), np.atleast_2d(np.asarray(hi, dtype=np.float64))
    B, M = lo.shape
    C = np.broadcast_to(np.asarray(C, dtype=np.float64), (B, M, M)).astype(real)
    rows = np.arange(B)
    lt, ht = lo.astype(real), hi.astype(real)
    if shift is not None:
        sh = np.broadcast_to(np.asarray(shift, dtype=np.float64), (B, M)).astype(real)
        lt, ht = lt - sh, ht - sh
    first = np.full(B, -1) if first is None else np.broadcast_to(np.asarray(first), (B,))
    v = C[:, np.arange(M), np.arange(M)].copy()
    s = np.zeros((B, M), dtype=real)
    W = np.zeros((B, M, M), dtype=real)                # [k][component]
    WS = np.zeros((B, M, M))                           # the scales of the entries, same layout
    remains = np.ones((B, M), dtype=bool)
    perm = np.zeros((B, M), dtype=np.int64)
    ok = np.ones(B, dtype=bool)
    margin = np.full((B, M), np.inf)
    ys = np.zeros((B, M), dtype=real)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        for i in range(M):
            sd = np.sqrt(v)
            a, b = (lt - s) / sd, (ht - s) / sd
            refl = a > 0
            d, e = _cdf(np.where(refl, -b, a), real), _cdf(np.where(refl, -a, b), real)
            w = np.where(lo < hi, e - d, real(0.0))
            key = np.where(remains & ~np.isnan(w), w, np.inf).astype(np.float64)
            kmin = np.where(remains, key, np.inf).min(axis=1)
            c = np.argmax(remains & (key == kmin[:, None]), axis=1)          # the lowest original index among the smallest
            forced = (first >= 0) & (i == 0)
            c = np.where(forced, first, c)
            if forced_perm is not None:
                c = np.asarray(forced_perm)[:, i]
            others = remains.copy()
            others[rows, c] = False
            second = np.where(others, key, np.inf).min(axis=1)
            wc = key[rows, c]
            m = np.where(wc > 0, (second - wc) / np.where(wc > 0, wc, 1.0), np.where(second > 0, np.inf, 0.0))
            margin[:, i] = np.where(forced | ~others.any(axis=1), np.inf, m)
            vc, sdc, ac, bc, wr = v[rows, c], sd[rows, c], a[rows, c], b[rows, c], w[rows, c]
            ok &= (vc > 0) & np.isfinite(vc.astype(np.float64))
            y = (_pdf(ac, real) - _pdf(bc, real)) / wr
            edge = np.where(ac > 0, ac, np.where(bc < 0, bc, real(0.0)))
            y = np.where((wr > 0) & np.isfinite(wr.astype(np.float64)) & ~np.isnan(y), y, edge)
            ys[:, i] = y
            perm[:, i] = c
            WS[rows, i, c] = ((np.abs(C[rows, c, c]) + np.sum(W[rows, :i, c] ** 2, axis=1)) / sdc).astype(np.float64)
            W[rows, i, c] = sdc
            remains = others
            row = W[rows, :, c]                        # [B, k]: L_c,k
            acc, mag = np.zeros((B, M), dtype=real), np.zeros((B, M))
            for k in range(i):
                t = W[:, k, :] * row[:, k, None]
                acc = acc + t
                mag += np.abs(t).astype(np.float64)
            ccol = C[rows, c, :]
            lji = (ccol - acc) / sdc[:, None]
            W[:, i, :] = np.where(remains, lji, W[:, i, :])
            WS[:, i, :] = np.where(remains, (np.abs(ccol).astype(np.float64) + mag) / sdc[:, None].astype(np.float64), WS[:, i, :])
            v = np.where(remains, v - lji * lji, v)
            s = np.where(remains, s + lji * y[:, None], s)
    L = np.stack([np.tril(W[b][:, perm[b]].T) for b in range(B)])
    scale = np.stack([np.tril(WS[b][:, perm[b]].T) for b in range(B)])
    return OrderResult(perm, L, ok, margin, scale, ys)


def permuted_covariance(C, perm):
    """[B, M, M]: C[perm][:, perm] of every box"""
    perm = np.asarray(perm, dtype=np.int64)
    B, M = perm.shape
    C = np.broadcast_to(np.asarray(C, dtype=np.float64), (B, M, M))
    return np.stack([C[b][np.ix_(perm[b], perm[b])] for b in range(B)])


# ---- the cases ------------------------------------------------------------------------------------------------------------------
class OrderCase:
    def __init__(self, name, C, lo, hi, shift=None, first=None):
        self.name = name
        self.C = np.asarray(C, dtype=np.float64)
        self.lo, self.hi = np.atleast_2d(np.asarray(lo, dtype=np.float64)), np.atleast_2d(np.asarray(hi, dtype=np.float64))
        self.lo, self.hi = np.broadcast_arrays(self.lo, self.hi)
        self.lo, self.hi = np.ascontiguousarray(self.lo), np.ascontiguousarray(self.hi)
        self.B, self.M = self.lo.shape
        self.shift = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
        self.first = None if first is None else np.ascontiguousarray(first, dtype=np.int32)

    def __repr__(self):
        return self.name


def _sym(F):
    c = F @ F.T
    return 0.5 * (c + c.T)


def equicorrelation(M, rho=0.5):
    c = np.full((M, M), rho)
    np.fill_diagonal(c, 1.0)
    return c


def ar_correlation(M, rho=0.8):
    i = np.arange(M)
    return rho ** np.abs(i[:, None] - i[None, :])


def _asc():
    return OrderCase("asc", equicorrelation(12), np.linspace(-2.0, 2.5, 12), np.inf)


def _ar():
    i = np.arange(12)
    lo = np.where(i % 2 == 0, -3.0, 1.5)
    return OrderCase("ar", ar_correlation(12), lo, np.where(i % 3 == 0, lo + 3.5, np.inf))


ASC, AR = _asc(), _ar()
TIE = OrderCase("tie", equicorrelation(12), np.full(12, -1.0), np.full(12, 1.0))

RANDOM_M = (1, 2, 3, 5, 12, 63, 64, 65, 128)
RANDOM_B = (1, 3, 70)
# seeds of the generator, chosen on the CPU so that the twin alone meets the condition of tests/test_box_order_cpu.py
RANDOM_SEED = 1000


def _random(M, B, seed=None):
    seed = RANDOM_SEED + 7 * M + B if seed is None else seed
    lo, hi = bp.boxes(M, B, seed)
    return OrderCase("random-M{}-B{}".format(M, B), _sym(bp.chol_factor(M, seed + 1)), lo, hi)


RANDOM_CASES = tuple(_random(M, B) for M in RANDOM_M for B in RANDOM_B)


def _special():
    out = []
    # a component of zero width (lo = hi): w = 0 exactly, y falls back to the edge nearer to 0
    lo, hi = bp.boxes(4, 3, 31)
    lo[:, 2], hi[:, 2] = np.array([0.7, -0.4, 0.0]), np.array([0.7, -0.4, 0.0])
    out.append(OrderCase("zero-width", _sym(bp.chol_factor(4, 32)), lo, hi))
    # a width that underflows: Phi(-40) is 0 in fp64
    lo, hi = bp.boxes(4, 2, 33)
    lo[:, 1], hi[:, 1] = np.array([40.0, -41.0]), np.array([41.0, -40.0])
    out.append(OrderCase("underflow", equicorrelation(4, 0.3), lo, hi))
    lo, hi = bp.boxes(5, 3, 35)
    out.append(OrderCase("forced-lead", _sym(bp.chol_factor(5, 36)), lo, hi, first=[2, -1, 4]))
    lo, hi = bp.boxes(5, 3, 37)
    F = bp.chol_factor(5, 38) * np.random.default_rng(39).uniform(0.3, 1.0, 5)[:, None]
    out.append(OrderCase("shift", _sym(F), lo, hi, shift=np.random.default_rng(40).uniform(-1.0, 1.0, (3, 5))))
    lo, hi = bp.boxes(6, 3, 41)
    out.append(OrderCase("stride", np.stack([_sym(bp.chol_factor(6, 42 + b)) for b in range(3)]), lo, hi))
    lo, hi = bp.boxes(65, 2, 45)
    out.append(OrderCase("stride-M65-forced-shift", np.stack([_sym(bp.chol_factor(65, 46 + b)) for b in range(2)]), lo, hi,
                         shift=np.random.default_rng(48).uniform(-0.5, 0.5, (2, 65)), first=[64, 0]))
    return tuple(out)


SPECIAL_CASES = _special()
NAMED_CASES = (ASC, AR, TIE)
ALL_CASES = NAMED_CASES + SPECIAL_CASES + RANDOM_CASES


@functools.lru_cache(maxsize=None)
def case_twin(case):
    return order_twin(case.C, case.lo, case.hi, case.shift, case.first)


def is_permutation(perm, M):
    return np.array_equal(np.sort(np.asarray(perm, dtype=np.int64), axis=1), np.broadcast_to(np.arange(M), np.shape(perm)))


# ---- the chain on a (re)ordered problem ------------------------------------------------------------------------------------------
def chain_stats(L, lo, hi, n, seeds=bp.SEEDS8, shift=None):
    """(prob, stderr, replicates) of one box from the chain twin on the project's own scrambled Sobol' points, coordinates 0 .. M-2"""
    M = np.shape(L)[0]
    reps = np.array([bp.tree_mean(bp.twin(L, lo, hi, shift, bp.points(s, list(range(M - 1)), 0, n, True))[0], 0, M) for s in seeds])
    return (*bp.summary(reps), reps)


def natural_and_ordered(case, n, seeds=bp.SEEDS8):
    """((prob, stderr, reps) in the caller's order, the same after `order_twin`) of box 0 of a case with one covariance"""
    natural = chain_stats(np.linalg.cholesky(case.C), case.lo[0], case.hi[0], n, seeds)
    t = case_twin(case)
    p = t.perm[0]
    return natural, chain_stats(t.L[0], case.lo[0][p], case.hi[0][p], n, seeds)


REFERENCE_N = 2 ** 16
REFERENCE_SEEDS = (100, 101)


def reference_probability(L, lo, hi, shift=None):
    """(prob, stderr) of one (re)ordered box from the chain twin at n = 2^16 under two seeds that no test gives the device; the
    standard error of two replicates is |r0 - r1| / 2"""
    return chain_stats(L, lo, hi, REFERENCE_N, REFERENCE_SEEDS, shift)[:2]
