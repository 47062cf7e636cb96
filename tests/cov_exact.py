"""Extended-precision reference of the moment covariance (LevelAccumulator COV: k_cov_accum*, k_cov_accum_t4*, k_cov_lin_mean,
k_spline_band_accum) -- TEST INFRASTRUCTURE, plain NumPy, a sibling of tests/accum_exact.py (whose transform, rows, log budget and
unit_errors it uses) and tests/gram_exact.py (whose fp64 identities it uses).  Nothing here imports the package, the device or the
oracle.

The rows phi(f), phi(c) [R, n] of the kept samples are those of accum_exact (fp64 transform contract; a NaN or a value outside the
domain in ANY component of fine or coarse drops the sample for all components).  Per level, component and kept sample, by the
DEFINITION and not by the kernel's identities,

    Y = phi(f) phi(f)^T - phi(c) phi(c)^T   (no coarse values: phi(f) phi(f)^T),      s = sum Y,      sp = sum Y o Y,

formed per sample in chunks of samples ([R, R, n] is never materialised; three expanded Grams would cancel in long double when
f ~ c).  Scales, as in gram_exact:

    a_i = |phi_i(f)| + |phi_i(c)| (+ the log budget E_i(f) + E_i(c) of accum_exact),   A = a_i a_j,   S = sum A,   SP = sum A^2,

which bound the terms of the definition and of the d / s form (d_i s_j + s_i d_j) / 2 alike.  Splines carry a budget E of the same
kind for the one rounding of the knot variable (spline_budget), to FIRST order: A = a_i a_j + a_i E_j + E_i a_j.  Without it a
sample on a knot puts the fp64 twins themselves 2^53 units away in the entries only that sample reaches; with (a + E)(a + E)
the term E_i E_j would dominate the scale (E reaches 170 at 128 splines while |B| <= 2/3).  Errors are in units of 2^-53 * scale
(accum_exact.unit_errors); a zero scale demands an exact zero -- for splines every entry with |i - j| > 3 and i, j >= 1.

Linearised entries (the mean of an eligible Legendre / Monomial covariance, the second moments of its levels without coarse
values): the library forms the entry as sum_k c_ijk (level sum of phi_k) over the 2 R - 1 (second moments: c2_ijk, 4 R - 3)
extended terms.  The reference VALUE stays the definition; the unit becomes sum_k |c_ijk| S_k with S_k the condition scale of
accum_exact.level_sums over the extended terms (lin_scales).

Twins (np.float64, calibration only -- no device result is ever compared with a twin):
    A    the definition in fp64 on the reference's own operation order (rows variant "A");
    B    rows with coefficients rounded beforehand (variant "B", where the family has one) through the kernel's identities
         1/2 (D^T S + S^T D), 1/4 (G1 + G1^T + 2 G2) with NumPy's own sums (gram_exact.xcov_identities);
    lin  fp64 level sums of the extended terms contracted with the coefficient table in ascending k (lin_contract): A from the rows
         of accum_exact (both variants), B from the route's own recurrences (legendre_monic_sums, chebyshev_sums with the second
         term window started by doubling, the connection table for the first 64 Chebyshev sums).
"""
import numpy as np

from tests import accum_exact as ax
from tests import gram_exact as gx

LD = ax.LD
_CHUNK = 1 << 21                          # elements of one [samples, R, R] block


class Sums:
    """n, n_rm [L]; s, sp, S, SP [L, M * R * R] (row (m * R + i) * R + j) in the working dtype"""


def kept_rows(desc, fine, coarse, dtype=LD, variant="A", budget=False):
    """keep [n] (the AND over the components of fine and coarse) and, over the kept samples, the rows pf, pc | None [M, R, n_keep]
    and the scale rows a = |pf| + |pc| + log budget [M, R, n_keep] of one level; with budget=True also the spline budget
    E [M, R, n_keep] | None, which enters the scales to first order only (definition)"""
    f = np.atleast_2d(np.asarray(fine, dtype=np.float64))
    c = None if coarse is None else np.atleast_2d(np.asarray(coarse, dtype=np.float64))
    keep = np.ones(f.shape[1], dtype=bool)
    for side in (f,) if c is None else (f, c):
        for m in range(side.shape[0]):
            keep &= ax.transform(desc, side[m], np.float64)[1]
    spline = desc.kind == ax.SPLINE and dtype is LD
    pf, Ef = ax._side(desc, f, keep, dtype, variant)
    a, E = np.abs(pf) + Ef, spline_budget(desc, f, keep) if spline else None
    pc = None
    if c is not None:
        pc, Ec = ax._side(desc, c, keep, dtype, variant)
        a = a + np.abs(pc) + Ec
        if spline:
            E = E + spline_budget(desc, c, keep)
    return (keep, pf, pc, a, E) if budget else (keep, pf, pc, a)


def spline_budget(desc, x, keep, h=2.0 ** -24):
    """E [M, R, n_keep] of a spline side: the move of B_k under one ulp of the knot variable v = u ns, in units of 2^-53:
    E_k = 2 |dB_k / du| |u| with u the position in the reference domain -- the counterpart of the log budget of accum_exact.  Any
    fp64 evaluation rounds v once; B_k next to the end of its support, ~ (v - k)^3 / 6, carries that rounding at 6 v / (v - k)
    times its own size, which sum |B_k| does not describe (a value ON a knot: ~1e-46 in long double, 0 in fp64).  The derivative
    is a central difference of accum_exact.rows in long double (one-sided at the ends of the domain): exact to ~h^2 for a
    piecewise cubic (it overestimates within h of a knot, where the true slope vanishes).  Non-zero only for the four B-splines
    of the sample's knot span, as fp64 arithmetic finds it, floor(fl(u ns)), and as the long double does (they differ for a value
    on a knot whose exact v lies ~1e-15 before it): an entry without common support keeps a scale of zero and must be exactly
    zero, except that such a knot sample leaves entries four apart a scale of the order of 1e-20."""
    r0, r1 = LD(desc.ref_domain[0]), LD(desc.ref_domain[1])
    out = np.zeros((x.shape[0], desc.size, int(keep.sum())), dtype=LD)
    step = LD(h) * (r1 - r0)
    for m in range(x.shape[0]):
        t = ax.transform(desc, x[m][keep], LD)[0]
        lo, hi = np.maximum(t - step, r0), np.minimum(t + step, r1)
        slope = (ax.rows(desc, hi, LD) - ax.rows(desc, lo, LD)) / (hi - lo)[None, :]
        ns = desc.size - 3
        k = np.arange(desc.size)[:, None]
        active = np.zeros(slope.shape, dtype=bool)
        for tt in (ax.transform(desc, x[m][keep], np.float64)[0], t):          # the span fp64 finds, and the long double's
            v = (tt - tt.dtype.type(desc.ref_domain[0])) / tt.dtype.type(desc.ref_domain[1] - desc.ref_domain[0]) * ns
            span = np.clip(np.floor(v), 0, ns - 1).astype(np.int64)
            active |= (k >= span[None, :]) & (k <= span[None, :] + 3) & (k >= 1)
        out[m] = np.where(active, 2 * np.abs(slope) * np.abs(t - r0)[None, :], LD(0))
    return out


def definition(F, C, a, dtype=LD, E=None):
    """s, sp, S, SP [R, R] of the rows F, C | None, a [R, n] of one component by the definition, per sample, in `dtype`.
    E [R, n] (splines): A = a_i a_j + a_i E_j + E_i a_j -- the budget to first order.  E is in units of 2^-53: an error
    2^-53 E_i in B_i moves the product by 2^-53 (a_i E_j + E_i a_j) + 2^-106 E_i E_j, and the last term is nothing in units of
    2^-53, while as E_i E_j it would be 10^4 times everything else at 128 splines."""
    R, n = F.shape
    iu, ju = np.triu_indices(R)                       # Y and A are symmetric by their definition: the upper triangle, mirrored
    acc = np.zeros((4, iu.size), dtype=dtype)
    b = max(1, _CHUNK // iu.size)
    for k0 in range(0, n, b):
        Fb = F[:, k0:k0 + b].astype(dtype)
        Y = Fb[iu] * Fb[ju]
        if C is not None:
            Cb = C[:, k0:k0 + b].astype(dtype)
            Y -= Cb[iu] * Cb[ju]
        ab = a[:, k0:k0 + b].astype(dtype)
        AA = ab[iu] * ab[ju]
        if E is not None:
            Eb = E[:, k0:k0 + b].astype(dtype)
            AA += ab[iu] * Eb[ju] + Eb[iu] * ab[ju]
        acc[0] += Y.sum(axis=-1)
        acc[2] += AA.sum(axis=-1)
        Y *= Y
        AA *= AA
        acc[1] += Y.sum(axis=-1)
        acc[3] += AA.sum(axis=-1)
    out = np.zeros((4, R, R), dtype=dtype)
    out[:, iu, ju] = acc
    out[:, ju, iu] = acc
    return out[0], out[1], out[2], out[3]


def cov_sums(desc, levels, dtype=LD, variant="A", identities=False, matrix=None):
    """levels: [(fine [M, n], coarse [M, n] | None)] raw values -> Sums.  dtype=LD: the reference (the definition on rows of
    variant "A").  np.float64: a twin -- the definition, or with identities=True the kernel's identities on rows of `variant`
    (its S, SP are zero: take the reference's).  matrix [Rout, R] (fp64): the covariance of psi = T phi (TransformedMoments),
    the matrix applied in `dtype`, the scales from |T| a."""
    L = len(levels)
    M = np.atleast_2d(levels[0][0]).shape[0]
    Ro = desc.size if matrix is None else matrix.shape[0]
    out = Sums()
    out.n, out.n_rm = np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64)
    out.s, out.sp, out.S, out.SP = (np.zeros((L, M, Ro * Ro), dtype=dtype) for _ in range(4))
    for l, (f, c) in enumerate(levels):
        keep, pf, pc, a, E = kept_rows(desc, f, c, dtype, variant, budget=True)
        out.n[l], out.n_rm[l] = keep.sum(), (~keep).sum()
        assert E is None or matrix is None
        for m in range(M):
            F, C, am = pf[m], None if pc is None else pc[m], a[m]
            if matrix is not None:
                T = np.asarray(matrix, dtype=np.float64).astype(dtype)
                F, C, am = _apply(T, F), None if C is None else _apply(T, C), _apply(np.abs(T), am)
            if identities:
                assert dtype is np.float64
                s, sp = gx.xcov_identities(F, C)
            else:
                s, sp, S, SP = definition(F, C, am, dtype, None if E is None else E[m])
                out.S[l, m], out.SP[l, m] = S.reshape(-1), SP.reshape(-1)
            out.s[l, m], out.sp[l, m] = s.reshape(-1), sp.reshape(-1)
    for key in ("s", "sp", "S", "SP"):
        setattr(out, key, getattr(out, key).reshape(L, M * Ro * Ro))
    return out


def _apply(T, X):
    """T [Ro, R] X [R, n] without BLAS, in the dtype of the operands (k ascending)"""
    out = np.zeros((T.shape[0], X.shape[1]), dtype=X.dtype)
    for k in range(T.shape[1]):
        out += T[:, k, None] * X[k][None, :]
    return out


def diff_gram_sums(desc, levels, matrix, dtype=LD, variant="A"):
    """The variance of TransformedMoments in MOMENTS mode (the difference Gram D^T D): per level and component
    s_i = sum_n (T d)_i, sp_i = sum_n (sum_k T_ik d_k)^2 with d = phi(f) - phi(c), and the scales sum_n (|T| a)_i and its square.
    -> Sums with s, sp, S, SP [L, M * Rout]"""
    L = len(levels)
    M = np.atleast_2d(levels[0][0]).shape[0]
    Ro = matrix.shape[0]
    T = np.asarray(matrix, dtype=np.float64).astype(dtype)
    out = Sums()
    out.n, out.n_rm = np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64)
    out.s, out.sp, out.S, out.SP = (np.zeros((L, M, Ro), dtype=dtype) for _ in range(4))
    for l, (f, c) in enumerate(levels):
        keep, pf, pc, a = kept_rows(desc, f, c, dtype, variant)
        out.n[l], out.n_rm[l] = keep.sum(), (~keep).sum()
        for m in range(M):
            d = _apply(T, pf[m] if pc is None else pf[m] - pc[m])
            b = _apply(np.abs(T), a[m])
            out.s[l, m], out.sp[l, m] = d.sum(axis=-1), (d * d).sum(axis=-1)
            out.S[l, m], out.SP[l, m] = b.sum(axis=-1), (b * b).sum(axis=-1)
    for key in ("s", "sp", "S", "SP"):
        setattr(out, key, getattr(out, key).reshape(L, M * Ro))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# linearised entries
# ---------------------------------------------------------------------------------------------------------------------------
def extended(desc, K):
    """the same moments object with K terms"""
    return ax.Desc(desc.kind, K, desc.domain, desc.ref_domain, desc.log, desc.safe_eval)


def check_table(table):
    """a linearisation table [K, R, R] of the library (host arithmetic, pinned to exact rationals by tests/test_linearize.py):
    non-negative, every (i, j) sums to one"""
    assert np.all(table >= 0) and np.max(np.abs(table.sum(axis=0) - 1.0)) < 5e-15
    return table


def lin_contract(table, sums):
    """sum_k table[k, i, j] sums[..., k] in ascending k, in the dtype of `sums` -> [..., R * R]"""
    K, R, _ = table.shape
    sums = np.asarray(sums)
    out = np.zeros(sums.shape[:-1] + (R * R,), dtype=sums.dtype)
    t = table.reshape(K, R * R).astype(sums.dtype)
    for k in range(K):
        out += t[k] * sums[..., k, None]
    return out


def lin_scales(desc, levels, table):
    """sum_k table[k, i, j] S_k per level and component [L, M * R * R]: S_k = the condition scale of accum_exact.level_sums over
    the K = table.shape[0] extended terms (long double)"""
    K, R, _ = check_table(table).shape
    ext = ax.level_sums(extended(desc, K), levels)
    M = np.atleast_2d(levels[0][0]).shape[0]
    return lin_contract(table, ext.S.reshape(len(levels), M, K)).reshape(len(levels), M * R * R)


def _kept_t(desc, levels):
    """per level and component the fp64 transformed kept values [(t_fine, t_coarse | None)]"""
    out = []
    for f, c in levels:
        f = np.atleast_2d(f)
        c = None if c is None else np.atleast_2d(c)
        keep = kept_rows(extended(desc, 1), f, c, np.float64)[0]
        out.append([(ax.transform(desc, f[m][keep], np.float64)[0], None if c is None else ax.transform(desc, c[m][keep], np.float64)[0])
                    for m in range(f.shape[0])])
    return out


def _diff_sums(step, start, tf, tc, first, count):
    """sum_n (term_k(f_n) - term_k(c_n)) for k = first .. first + count - 1 of a three-term recurrence: start(t) -> state,
    step(k, state) -> (state, term_k)"""
    states = [start(t) for t in ((tf,) if tc is None else (tf, tc))]
    out = np.empty(count)
    for k in range(first, first + count):
        terms = []
        for i, st in enumerate(states):
            states[i], term = step(k, st)
            terms.append(term)
        out[k - first] = np.sum(terms[0] if tc is None else terms[0] - terms[1])
    return out


def legendre_monic_sums(tf, tc, K):
    """fp64 (NumPy, no FMA) sums of P_k(f) - P_k(c), k < K, by the scaled monic recurrence of the matrix kernel:
    P_k = c_k q_k, q_k = 2 t q_{k-1} - 4 g_k q_{k-2}, g_k = (k-1)^2 / ((2k-1)(2k-3)), c_k = c_{k-1} (2k-1) / (2k)"""
    def start(t):
        return (2.0 * t, np.zeros_like(t), np.ones_like(t))

    def step(k, st):
        x2, q2, q1 = st
        if k == 0:
            return st, q1
        g4 = 0.0 if k < 2 else 4.0 * ((k - 1) * (k - 1) / ((2 * k - 1) * (2 * k - 3)))
        q = x2 * q1 - g4 * q2
        return (x2, q1, q), q

    raw = _diff_sums(step, start, tf, tc, 0, K)
    c = 1.0
    for k in range(1, K):
        c = c * (2 * k - 1) / (2 * k)
        raw[k] *= c
    return raw


def chebyshev_sums(tf, tc, K, jump=True):
    """fp64 sums of T_k(f) - T_k(c), k < K: T_k = 2 t T_{k-1} - T_{k-2} from T_0, T_1; with jump, the terms from 64 on restart
    from (T_62, T_63) reached by six doublings T_2m = 2 T_m^2 - 1, T_2m+1 = 2 T_m T_m+1 - t and two steps back, as the kernel's
    second term window starts them"""
    def start(t):
        return (2.0 * t, None, None, t)

    def step(k, st):
        x2, p2, p1, t = st
        term = np.ones_like(t) if k == 0 else t if k == 1 else x2 * p1 - p2
        return (x2, p1, term, t), term

    def start64(t):
        x2 = 2.0 * t
        a, b = t.copy(), x2 * t - 1.0
        for _ in range(6):
            a2 = 2.0 * a
            a, b = a2 * a - 1.0, a2 * b - t
        p1 = x2 * a - b                               # T_63
        return (x2, x2 * p1 - a, p1, t)               # (.., T_62, T_63, ..)

    if not jump or K <= 64:
        return _diff_sums(step, start, tf, tc, 0, K)
    return np.concatenate([_diff_sums(step, start, tf, tc, 0, 64), _diff_sums(step, start64, tf, tc, 64, K - 64)])


def route_level_sums(desc, levels, K, sums):
    """[L, M, K] of sums(t_fine, t_coarse | None, K) over the kept samples of every level and component (Legendre moments: the
    reference domain is [-1, 1])"""
    assert desc.kind == ax.LEGENDRE
    return np.array([[sums(tf, tc, K) for tf, tc in level] for level in _kept_t(desc, levels)])
