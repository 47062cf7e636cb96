"""The coefficient tables for level sums of CHEBYSHEV polynomials (mlmc_linearization_table, squares = 2 | 3): the inner
accumulators of a Legendre covariance sum T_k instead of P_k (one FMA per term), and the exact connection
P_k = sum_m a_km T_m,  a_{k,|k-2j|} += g_j g_{k-j},  g_j = (2j - 1)!! / (2j)!!,  is folded into the tables on the host:
c'_ijm = sum_k c_ijk a_km.  Host arithmetic behind the C ABI: no GPU here.

- small sizes against exact rationals (Adams' formula and the connection in Fractions);
- full sizes: the properties the accumulators rest on (non-negative, bit-symmetric, rows sum to one, structural zeros, exact
  counts through c'_00m = delta_m0, squares' i = 0 rows = the product table's);
- a NumPy emulation of both routes (sums of Legendre / of Chebyshev polynomials, contracted with their tables) on seeded samples
  of the benchmark's synthetic workload, against an extended-precision reference, under the gates of the GPU parity test:
  1e-12 of sqrt(sp n) for the means, 1e-11 for the level-0 second moments.
"""
from fractions import Fraction
from math import factorial

import numpy as np
import pytest

DOMAIN = (-3.7190164854556804, 3.7190164854556804)


def _lib_table(R, squares):
    from mlmc_amd import _lib
    K = 4 * R - 3 if squares in (1, 3) else 2 * R - 1
    out = np.empty(K * R * R)
    _lib.check(_lib.load().mlmc_linearization_table(_lib.LEGENDRE, R, squares, _lib.ptr(out), out.size))
    return out.reshape(K, R, R)


def _exact_legendre_products(R):
    """c_ijk as Fractions by Adams' formula with exact factorial ratios."""
    def A(n):                                        # (2n - 1)!! / n! = (2n)! / (2^n n!^2)
        return Fraction(factorial(2 * n), 2 ** n * factorial(n) ** 2)
    c = {}
    for i in range(R):
        for j in range(R):
            for k in range(abs(i - j), i + j + 1, 2):
                s = (i + j + k) // 2
                c[i, j, k] = Fraction(2 * k + 1, 2 * s + 1) * A(s - i) * A(s - j) * A(s - k) / A(s)
    return c


def _exact_connection(K):
    """a[k][m] of P_k = sum_m a_km T_m as Fractions."""
    g = [Fraction(1)]
    for j in range(1, K):
        g.append(g[-1] * Fraction(2 * j - 1, 2 * j))
    a = [dict() for _ in range(K)]
    for k in range(K):
        for j in range(k + 1):
            m = abs(k - 2 * j)
            a[k][m] = a[k].get(m, Fraction(0)) + g[j] * g[k - j]
    return a


def test_connection_is_the_change_of_basis():
    """P_k(t) = sum_m a_km T_m(t) at a few points, rows sum to one, parity kept."""
    a = _exact_connection(12)
    t = np.array([-0.93, -0.2, 0.0, 0.41, 1.0])
    for k in range(12):
        assert sum(a[k].values()) == 1 and all(v > 0 and (m - k) % 2 == 0 and m <= k for m, v in a[k].items())
        P = np.polynomial.legendre.legval(t, [0] * k + [1])
        T = sum(float(v) * np.polynomial.chebyshev.chebval(t, [0] * m + [1]) for m, v in a[k].items())
        assert np.max(np.abs(P - T)) < 1e-14


@pytest.mark.parametrize("R", [1, 2, 5, 9])
def test_chebyshev_tables_against_exact_rationals(R):
    """Products: the extended-precision sum is rounded once more to double -- within one unit in the last place of the exact value
    (and exactly zero where the exact value is); squares: 4e-16 max(exact, 1e-3), the tolerance of the Legendre tables' test."""
    c = _exact_legendre_products(2 * R)              # products of products need the table of the doubled size
    a = _exact_connection(4 * R - 3)
    t1 = _lib_table(R, 2)
    t2 = _lib_table(R, 3)
    assert t1.shape == (2 * R - 1, R, R) and t2.shape == (4 * R - 3, R, R)
    for i in range(R):
        for j in range(R):
            row = {k: c[i, j, k] for k in range(abs(i - j), i + j + 1, 2)}
            ch = {}
            for k, ck in row.items():
                for m, akm in a[k].items():
                    ch[m] = ch.get(m, Fraction(0)) + ck * akm
            for m in range(2 * R - 1):
                exact = float(ch.get(m, Fraction(0)))
                assert abs(t1[m, i, j] - exact) <= np.spacing(exact), (i, j, m, t1[m, i, j], exact)
                if m not in ch:
                    assert t1[m, i, j] == 0.0
            sq = {}
            for k1, ca in row.items():
                for k2, cb in row.items():
                    for k in range(abs(k1 - k2), k1 + k2 + 1, 2):
                        sq[k] = sq.get(k, Fraction(0)) + ca * cb * c[k1, k2, k]
            ch2 = {}
            for k, ck in sq.items():
                for m, akm in a[k].items():
                    ch2[m] = ch2.get(m, Fraction(0)) + ck * akm
            for m in range(4 * R - 3):
                exact = float(ch2.get(m, Fraction(0)))
                assert abs(t2[m, i, j] - exact) <= 4e-16 * max(exact, 1e-3), (i, j, m, t2[m, i, j], exact)
                if m not in ch2:
                    assert t2[m, i, j] == 0.0


@pytest.mark.parametrize("R", [17, 64])
def test_chebyshev_tables_properties(R):
    t1 = _lib_table(R, 2)
    t2 = _lib_table(R, 3)
    for t in (t1, t2):
        assert np.all(t >= 0) and np.array_equal(t, t.transpose(0, 2, 1))
        assert np.max(np.abs(t.sum(axis=0) - 1.0)) < 5e-15
    # zeros where parity or degree forbid an entry: T_m appears in P_i P_j only for m <= i + j, m = i + j (mod 2); in (P_i P_j)^2
    # only for even m <= 2 (i + j)
    I, J = np.meshgrid(np.arange(R), np.arange(R), indexing="ij")
    for m in range(2 * R - 1):
        assert not t1[m][(I + J < m) | ((I + J - m) % 2 == 1)].any()
    assert not t2[1::2].any()
    for m in range(4 * R - 3):
        assert not t2[m][2 * (I + J) < m].any()
    # unlike the Legendre coefficients (zero below |i - j|) the permitted entries are all there
    assert np.all(t1[0][(I + J) % 2 == 0] > 0)
    # exact counts: T_0 = P_0 = 1
    for t in (t1, t2):
        assert t[0, 0, 0] == 1.0 and not t[1:, 0, 0].any()
    # (P_0 P_j)^2 = P_j^2: the squares' rows with i = 0 are the product table's, bit for bit
    for j in range(R):
        assert np.array_equal(t2[:2 * R - 1, 0, j], t1[:, j, j]) and not t2[2 * R - 1:, 0, j].any()
    # the Legendre tables (squares = 0 | 1) composed with the connection in double agree to rounding
    K2 = 4 * R - 3
    a = np.zeros((K2, K2))
    for k, rowa in enumerate(_exact_connection(K2)):
        for m, v in rowa.items():
            a[k, m] = float(v)
    assert np.max(np.abs(np.einsum("kij,km->mij", _lib_table(R, 0), a[:2 * R - 1, :2 * R - 1]) - t1)) < 1e-14
    assert np.max(np.abs(np.einsum("kij,km->mij", _lib_table(R, 1), a) - t2)) < 1e-14


def test_chebyshev_table_argument_checks():
    from mlmc_amd import _lib
    lib = _lib.load()
    out = np.empty(64)
    for args in ((_lib.MONOMIAL, 2, 2, _lib.ptr(out), 64),      # the Chebyshev sums belong to Legendre moments
                 (_lib.MONOMIAL, 2, 3, _lib.ptr(out), 64),
                 (_lib.LEGENDRE, 129, 2, _lib.ptr(out), 64),
                 (_lib.LEGENDRE, 65, 3, _lib.ptr(out), 64),     # squares: at most 64 moments
                 (_lib.LEGENDRE, 2, 4, _lib.ptr(out), 64),      # 0 .. 3
                 (_lib.LEGENDRE, 2, -1, _lib.ptr(out), 64),
                 (_lib.LEGENDRE, 3, 2, _lib.ptr(out), 44)):     # needs 5 * 9 = 45 doubles
        assert lib.mlmc_linearization_table(*args) != 0
        assert lib.mlmc_last_error().decode() != ""
    assert lib.mlmc_linearization_table(_lib.LEGENDRE, 2, 2, _lib.ptr(out), 12) == 0
    # P_1^2 = 1/3 P_0 + 2/3 P_2 = 1/3 + 2/3 (1/4 + 3/4 T_2) = 1/2 T_0 + 1/2 T_2
    assert np.array_equal(out[:12].reshape(3, 2, 2)[:, 1, 1], [0.5, 0.0, 0.5])


def test_both_routes_on_the_benchmark_samples():
    """R = 64, 5 levels x 6e4 seeded samples of the benchmark's synthetic workload.  Level sums of the extended moments in
    double with NumPy (multiply and subtract rounded separately: no FMA), of Legendre polynomials by the accumulators' scaled
    monic recurrence and of Chebyshev polynomials by T_k = 2t T_{k-1} - T_{k-2}, the terms from 128 on started from the doubling
    identities as in the kernel's second window; each contracted with its tables.  Reference:
    Legendre values, their products and all sums in extended precision.  Gates of the GPU parity test
    (test_covariance_mean_through_the_product_linearisation): means within 1e-12 of sqrt(sp n), level-0 second moments within
    1e-11 (relative, entries below 1e-3 of the level's largest measured against that).  Measured when the tables were introduced:
    Chebyshev 1.5e-15 and 1.9e-14, Legendre 6.8e-16 and 7.5e-15."""
    from oracle import oracle_np as onp
    assert np.finfo(np.longdouble).eps < 2e-19       # the reference (like the library's tables) needs the 80-bit format
    R, L, N = 64, 5, 60000
    K1, K2 = 2 * R - 1, 4 * R - 3
    steps = [s[0] for s in onp.determine_level_parameters(L, [0.5, 0.01])]
    shift, scale = DOMAIN[0], 2.0 / (DOMAIN[1] - DOMAIN[0])
    ld = np.longdouble

    def transform(x):
        return (x - shift) * scale + (-1.0)          # two roundings, like the kernels

    def legendre_ld(t, K):
        P = np.empty((K, t.size), dtype=ld)
        tl = t.astype(ld)
        P[0] = 1
        P[1] = tl
        for k in range(2, K):
            P[k] = ((2 * k - 1) * tl * P[k - 1] - (k - 1) * P[k - 2]) / k
        return P

    def legendre_terms(t, K):                        # device form: q_k = 2t q_{k-1} - 4 g_k q_{k-2}, P_k = c_k q_k
        x2 = 2.0 * t
        q2, q1 = np.zeros_like(t), np.ones_like(t)
        c = 1.0
        yield c, q1
        for k in range(1, K):
            g4 = 0.0 if k < 2 else 4.0 * ((k - 1) * (k - 1) / ((2 * k - 1) * (2 * k - 3)))
            q = x2 * q1 - g4 * q2
            q2, q1 = q1, q
            c = c * (2 * k - 1) / (2 * k)
            yield c, q

    def chebyshev_terms(t, K):
        x2 = 2.0 * t
        p2, p1 = np.ones_like(t), t.copy()
        yield 1.0, p2
        yield 1.0, p1
        for k in range(2, K):
            if k == 128:                             # second window, as the kernel starts it (TermGen::jump128): (T_1, T_2) ->
                a, b = t.copy(), x2 * t - 1.0        # (T_128, T_129) by T_2n = 2 T_n^2 - 1, T_2n+1 = 2 T_n T_n+1 - t, two steps back
                for _ in range(7):
                    a2 = 2.0 * a
                    a, b = a2 * a - 1.0, a2 * b - t
                p1 = x2 * a - b                      # T_127
                p2 = x2 * p1 - a                     # T_126
            q = x2 * p1 - p2
            p2, p1 = p1, q
            yield 1.0, q

    def level_sums(terms, tf, tc, K):                # sum_n (phi_k(f_n) - phi_k(c_n)), the difference taken per sample
        if tc is None:
            return np.array([c * np.sum(v) for c, v in terms(tf, K)])
        return np.array([c * np.sum(vf - vc) for (c, vf), (_, vc) in zip(terms(tf, K), terms(tc, K))])

    tabs = {"legendre": (_lib_table(R, 0), _lib_table(R, 1), legendre_terms),
            "chebyshev": (_lib_table(R, 2), _lib_table(R, 3), chebyshev_terms)}
    worst = {name: [0.0, 0.0] for name in tabs}
    for l in range(L):
        f, c = onp.synth_level_samples(l, N, steps)
        tf = transform(f)
        keep = (tf >= -1.0) & (tf <= 1.0)
        tc = None
        if c is not None:
            tc = transform(c)
            keep &= (tc >= -1.0) & (tc <= 1.0)
            tc = tc[keep]
        tf = tf[keep]
        n = tf.size
        # reference: sum_n (f_i f_j - c_i c_j) = (F F^T - C C^T)_ij; sum_n (f_i f_j - c_i c_j)^2 from the squared values likewise
        F = legendre_ld(tf, R)
        s_ref = F @ F.T
        F2 = F * F
        sp_ref = F2 @ F2.T
        if tc is not None:
            C = legendre_ld(tc, R)
            s_ref = s_ref - C @ C.T
            C2, FC = C * C, F * C
            sp_ref = sp_ref + C2 @ C2.T - 2 * (FC @ FC.T)
        gate_scale = np.sqrt(np.abs(sp_ref) * n).astype(float) + 1e-300
        for name, (t1, t2, terms) in tabs.items():
            S = level_sums(terms, tf, tc, K2 if tc is None else K1)
            s = np.tensordot(S[:K1], t1, axes=(0, 0))
            worst[name][0] = max(worst[name][0], float(np.max(np.abs(s - s_ref) / gate_scale)))
            if tc is None:
                sp = np.tensordot(S, t2, axes=(0, 0))
                big = float(np.max(np.abs(sp_ref)))
                rel = np.abs(sp - sp_ref) / np.maximum(np.abs(sp_ref), 1e-3 * big)
                worst[name][1] = max(worst[name][1], float(np.max(rel)))
    print("means / sqrt(sp n), level-0 second moments (relative):", worst)
    for name in tabs:
        assert worst[name][0] < 1e-12, (name, worst[name])
        assert worst[name][1] < 1e-11, (name, worst[name])
