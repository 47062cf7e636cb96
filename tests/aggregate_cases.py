"""References, twin and cases of the scenario-aggregate entries (mlmc_scenario_aggregates, mlmc_rows_weighted_sums); test helpers, not
product code.

aggregates_reference: what mlmc_scenario_aggregates must return bit for bit, in NumPy on whole columns.
chain_exact: one linear chain in exact rational arithmetic with a correct rounding after every product and every sum.
weighted_sums_ld / weighted_sums_exact: the sums of mlmc_rows_weighted_sums in long double / in exact rationals.
weighted_sums_twin: the sums in fp64 in the ORDER of the kernel (include/mlmc_hip.h): it tells here, without a device, how far that
order lies from the long-double reference, which fixes the gate of the device test:

    worst distance of the twin over the cases of `sum_cases()` (tests/test_aggregates_cpu.py measures and asserts both):
        first sums  (sum f, sum f d and the tail sums)   in units of 2^-53 sum f |d| (sum f for the weights):  TWIN_WORST_FIRST
        second sums (sum f d^2)                          in units of 2^-53 sum f d^2:                          TWIN_WORST_SECOND
    gate = 4 x that worst, rounded up to a power of two (the margin allows for another summation order on the device):  GATE_*
    the device's own worst on the same cases (tests/test_gpu_aggregates.py prints it):  DEVICE_WORST_*
"""
from fractions import Fraction

import numpy as np

AGG_MAX, AGG_MIN, AGG_COUNT, AGG_ARGMAX, AGG_ARGMIN = 1, 2, 4, 8, 16
EXTRA_BITS = (AGG_MAX, AGG_MIN, AGG_COUNT, AGG_ARGMAX, AGG_ARGMIN)

TWIN_WORST_FIRST, TWIN_WORST_SECOND = 1.95, 2.28       # measured by test_twin_distance_and_gate (asserted there)
GATE_FIRST, GATE_SECOND = 8.0, 16.0                     # 4 x worst, rounded up to a power of two
DEVICE_WORST_FIRST, DEVICE_WORST_SECOND = 1.944, 2.279  # one MI355X, the 108 cases: the twin's own figures (1.944, 2.279), same order


# ---- mlmc_scenario_aggregates -------------------------------------------------------------------------------------------------
def aggregates_reference(x, W, members, lower, upper, extras):
    """x [S, M, n], W [A, M] or None, members [M] or None, lower / upper [M] or None -> [S, Q, n]"""
    x = np.asarray(x, dtype=np.float64)
    S, M, n = x.shape
    rows = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0 if W is None else len(W)):
            acc = np.zeros((S, n))
            for m in range(M):
                acc = acc + W[a][m] * x[:, m, :]
            rows.append(acc)
        if extras & (AGG_MAX | AGG_MIN | AGG_ARGMAX | AGG_ARGMIN):
            mem = np.arange(M) if members is None else np.flatnonzero(members)
            sub = x[:, mem, :]
            if n:
                amax, amin = np.argmax(sub, axis=1), np.argmin(sub, axis=1)
            else:
                amax = amin = np.zeros((S, 0), dtype=np.int64)
            vmax = np.take_along_axis(sub, amax[:, None, :], axis=1)[:, 0, :]
            vmin = np.take_along_axis(sub, amin[:, None, :], axis=1)[:, 0, :]
        if extras & AGG_COUNT:
            lo = np.full(M, -np.inf) if lower is None else np.asarray(lower, dtype=np.float64)
            hi = np.full(M, np.inf) if upper is None else np.asarray(upper, dtype=np.float64)
            constrained = np.isfinite(lo) | np.isfinite(hi)
            inside = (lo[None, :, None] < x) & (x < hi[None, :, None])
            count = np.sum(constrained[None, :, None] & ~inside, axis=1).astype(np.float64)
    if extras & AGG_MAX:
        rows.append(vmax)
    if extras & AGG_MIN:
        rows.append(vmin)
    if extras & AGG_COUNT:
        rows.append(count)
    if extras & AGG_ARGMAX:
        rows.append(mem[amax].astype(np.float64))
    if extras & AGG_ARGMIN:
        rows.append(mem[amin].astype(np.float64))
    return np.stack(rows, axis=1) if rows else np.zeros((S, 0, n))


def _rounded(op, a, b):
    """fl(a op b) for doubles a, b: exact rationals and ONE correct rounding (int / int is correctly rounded); IEEE rules where an operand
    is not finite"""
    if not (np.isfinite(a) and np.isfinite(b)):
        with np.errstate(invalid="ignore"):
            return float(np.float64(a) * np.float64(b)) if op == "*" else float(np.float64(a) + np.float64(b))
    r = Fraction(a) * Fraction(b) if op == "*" else Fraction(a) + Fraction(b)
    if r == 0:                                              # the sign of an exact zero: IEEE's own rule
        return float(np.float64(a) * np.float64(b)) if op == "*" else float(np.float64(a) + np.float64(b))
    try:
        return r.numerator / r.denominator
    except OverflowError:
        return np.inf if r > 0 else -np.inf


def chain_exact(w, col):
    """acc = +0.0; acc = fl(acc + fl(w[m] * col[m])) for m ascending"""
    acc = 0.0
    for wm, xm in zip(w, col):
        acc = _rounded("+", acc, _rounded("*", float(wm), float(xm)))
    return acc


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def scenario_inputs(S, M, n, seed):
    """x [S, M, n]: normal draws with, where the shape has room, a column holding a NaN, one with NaNs in two components, +inf and -inf,
    equal maxima and minima, and -0.0 next to +0.0 as the extremes"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((S, M, n))
    if n == 0:
        return x
    col = lambda k: (k * 7 + 3) % n
    x[:, M // 2, col(0)] = np.nan
    x[:, 0, col(1)] = np.nan
    x[:, M - 1, col(1)] = np.nan
    x[:, M // 3, col(2)] = np.inf
    x[:, (2 * M) // 3, col(3)] = -np.inf
    x[:, :, col(4)] = np.minimum(x[:, :, col(4)], 0.25)
    x[:, 0, col(4)] = x[:, M - 1, col(4)] = x[:, M // 2, col(4)] = 0.25            # equal maxima
    x[:, :, col(5)] = np.maximum(x[:, :, col(5)], -0.5)
    x[:, M - 1, col(5)] = x[:, M // 2, col(5)] = -0.5                               # equal minima
    x[:, :, col(6)] = -np.abs(x[:, :, col(6)]) - 1.0
    x[:, 0, col(6)] = -0.0                                                         # the maximum: -0.0 first, then +0.0
    if M > 1:
        x[:, M - 1, col(6)] = 0.0
    x[:, :, col(7)] = np.abs(x[:, :, col(7)]) + 1.0
    x[:, 0, col(7)] = 0.0                                                          # the minimum: +0.0 first, then -0.0
    if M > 1:
        x[:, M - 1, col(7)] = -0.0
    x[:, M // 2, col(8)] = np.inf                                                  # 0 * inf under a zero weight
    return x


def scenario_weights(A, M, seed):
    if A == 0:
        return None
    W = np.random.default_rng(seed).uniform(-2.0, 2.0, (A, M))
    W[0, M // 2] = 0.0                                                             # meets the +inf of scenario_inputs: NaN
    return np.ascontiguousarray(W)


def scenario_members(kind, M):
    if kind == "all":
        return None
    mem = np.zeros(M, dtype=np.uint8)
    if kind == "one":
        mem[M - 1] = 1
    else:
        mem[1 if M > 1 else 0::2] = 1              # alternating, component 0 (which holds a NaN) is not a member
    return mem


def scenario_limits(kind, M):
    if kind == "finite":
        return np.linspace(-1.0, -0.2, M), np.linspace(0.3, 1.5, M)
    if kind == "one-sided":
        lo, hi = np.full(M, -np.inf), np.full(M, np.inf)
        lo[0::3] = -0.5
        hi[1::3] = 0.75
        return lo, hi
    return None, None


# ---- mlmc_rows_weighted_sums --------------------------------------------------------------------------------------------------
RW_THREADS, RW_MAX_BLOCKS, RW_MIN_PER = 256, 1024, 2048


def rw_per(n):
    per = -(-n // RW_MAX_BLOCKS)
    per = -(-per // RW_THREADS) * RW_THREADS
    return max(per, RW_MIN_PER)


def _terms(y, f, c, t, lower, dtype):
    """per column: (keep, the 3 + 2 P term rows of the sums) in `dtype`; products in the order of the kernel: (f d), (f d) d"""
    y = np.asarray(y, dtype=np.float64)
    fv = np.ones_like(y) if f is None else np.asarray(f, dtype=np.float64)
    keep = ~np.isnan(y) & ~np.isnan(fv)
    w = np.where(keep, fv, 0.0).astype(dtype)
    if dtype == np.float64:
        d = np.where(keep, y - c, 0.0)
    else:
        d = np.where(keep, y.astype(dtype) - dtype(c), dtype(0))
    wd = w * d
    rows = [w, wd, wd * d]
    for tk in t:
        with np.errstate(invalid="ignore"):
            ind = keep & ((y <= tk) if lower else (y >= tk))
        rows.append(np.where(ind, w, dtype(0)))
        rows.append(np.where(ind, wd, dtype(0)))
    return keep, rows


def weighted_sums_ld(y, f, c, t, lower=False):
    """(n_used, sums [3 + 2 P] as long doubles): the sums of one row with every product and sum in long double"""
    keep, rows = _terms(y, f, c, t, lower, np.longdouble)
    return int(keep.sum()), np.array([np.sum(r, dtype=np.longdouble) for r in rows], dtype=np.longdouble)


def weighted_sums_exact(y, f, c, t, lower=False):
    """the same sums as exact rationals (finite data)"""
    y = np.asarray(y, dtype=np.float64)
    fv = np.ones_like(y) if f is None else np.asarray(f, dtype=np.float64)
    out = [Fraction(0)] * (3 + 2 * len(t))
    for yi, fi in zip(y, fv):
        if np.isnan(yi) or np.isnan(fi):
            continue
        w, d = Fraction(float(fi)), Fraction(float(yi)) - Fraction(float(c))
        out[0] += w
        out[1] += w * d
        out[2] += w * d * d
        for k, tk in enumerate(t):
            if (yi <= tk) if lower else (yi >= tk):
                out[3 + 2 * k] += w
                out[4 + 2 * k] += w * d
    return out


def _block_sum(terms):
    """one block's sum in the order of the kernel: thread t adds its columns ascending, wave butterfly, the four waves in order"""
    trips = -(-terms.size // RW_THREADS)
    buf = np.zeros(trips * RW_THREADS)                   # + 0.0 for the columns a thread does not have: changes no bit
    buf[:terms.size] = terms
    v = np.zeros(RW_THREADS)
    for row in buf.reshape(trips, RW_THREADS):
        v = v + row
    lanes = np.arange(64)
    w = []
    for k in range(4):
        l = v[64 * k:64 * k + 64].copy()
        for off in (32, 16, 8, 4, 2, 1):
            l = l + l[lanes ^ off]
        w.append(l[0])
    return ((w[0] + w[1]) + w[2]) + w[3]


def weighted_sums_twin(y, f, c, t, lower=False):
    """(n_used, sums [3 + 2 P]) in fp64 in the order of the kernel"""
    keep, rows = _terms(y, f, c, t, lower, np.float64)
    n, per = keep.size, rw_per(keep.size)
    out = np.zeros(len(rows))
    for k, r in enumerate(rows):
        s = 0.0
        for s0 in range(0, n, per):
            s = s + _block_sum(r[s0:s0 + per])
        out[k] = s
    return int(keep.sum()), out


def sum_units(y, f, c):
    """(sum f, sum f |d|, sum f d^2) in long double over the used columns: the units of the distances"""
    y = np.asarray(y, dtype=np.float64)
    fv = np.ones_like(y) if f is None else np.asarray(f, dtype=np.float64)
    keep = ~np.isnan(y) & ~np.isnan(fv)
    w = np.where(keep, fv, 0.0).astype(np.longdouble)
    d = np.where(keep, y.astype(np.longdouble) - np.longdouble(c), np.longdouble(0))
    return float(np.sum(w)), float(np.sum(w * np.abs(d))), float(np.sum(w * d * d))


def distances(got, ref, units):
    """(worst first-sum distance, second-sum distance) of sums [3 + 2 P] from the long-double ones, in the units of the module text"""
    sf, sfd, sfd2 = units
    eps = 2.0 ** -53
    first = 0.0
    for k in range(len(got)):
        if k == 2:
            continue
        unit = eps * (sf if k == 0 or (k >= 3 and k % 2 == 1) else sfd)
        err = abs(float(np.longdouble(got[k]) - ref[k]))
        first = max(first, err / unit if unit > 0 else (0.0 if err == 0 else np.inf))
    err2 = abs(float(np.longdouble(got[2]) - ref[2]))
    second = err2 / (eps * sfd2) if sfd2 > 0 else (0.0 if err2 == 0 else np.inf)
    return first, second


SUM_SIZES = (1, 63, 64, 65, 255, 256, 257, 4097, 20011)


def sum_row(kind, n, seed):
    """one data row: 'offset' = 1e6 + 1e-3 z (a mean far above the spread), 'lognormal' = exp(z)"""
    z = np.random.default_rng(seed).standard_normal(n)
    return 1e6 + 1e-3 * z if kind == "offset" else np.exp(z)


def sum_weights(kind, n, seed):
    """None, 'random' weights in [0, 1], or 'zeros': the same with exact zeros at a third of the columns"""
    if kind is None:
        return None
    rng = np.random.default_rng(seed + 1000)
    f = rng.uniform(0.0, 1.0, n)
    if kind == "zeros":
        f[rng.uniform(size=n) < 1.0 / 3.0] = 0.0
    return f


def row_thresholds(y):
    """below, inside, above the data, and equal to a data value"""
    y = y[~np.isnan(y)]
    return np.array([y.min() - 1.0, np.median(y) + 1e-7 * abs(np.median(y)), y.max() + 1.0, np.sort(y)[y.size // 3]])


def sum_cases():
    """(name, y, f, c, t): every data kind, size and weight kind, about 0 (the first call of row_statistics) and about the weighted mean
    (the second)"""
    for data in ("offset", "lognormal"):
        for i, n in enumerate(SUM_SIZES):
            for j, wk in enumerate((None, "random", "zeros")):
                y, f = sum_row(data, n, 100 * i + j), sum_weights(wk, n, 100 * i + j)
                fv = np.ones(n) if f is None else f
                t = row_thresholds(y)
                yield "{}-n{}-{}-c0".format(data, n, wk), y, f, 0.0, t
                if fv.sum() > 0:
                    yield "{}-n{}-{}-mean".format(data, n, wk), y, f, float(np.sum(fv * y) / fv.sum()), t
