"""The connection from Legendre to Chebyshev polynomials, T_m = sum_{k <= m} b_mk P_k (mlmc_chebyshev_connection_table): a
covariance with variances of 49..64 Legendre moments takes the first 64 Chebyshev level sums of its pair levels from the Legendre
difference sums that the matrix kernel accumulates on the side, S[T_m] = sum_k b_mk S[P_k], and walks only the terms from 64 on in
the auxiliary pass.  Host arithmetic behind the C ABI: no GPU here.

- the exported table against exact rationals: the inverse of the exact a_km (P_k = sum_m a_km T_m) of test_chebyshev_tables_cpu;
- the properties the accumulators rest on: b_00 = 1 and b_0k = 0 exactly (exact zeros in the P_0 P_0 entries of the pair levels),
  parity zeros, rows that sum to one, a positive diagonal over non-positive entries;
- argument checks;
- a NumPy emulation of the route on seeded pairs of the benchmark's synthetic workload against an extended-precision reference,
  under the gate of the GPU parity tests: 1e-12 of sqrt(sp n).
"""
from fractions import Fraction

import numpy as np
import pytest

from tests import cov_exact as cx
from tests.test_chebyshev_tables_cpu import DOMAIN, _exact_connection, _lib_table

M = 64


def _lib_connection(m):
    from mlmc_amd import _lib
    out = np.full(m * m, np.nan)
    _lib.check(_lib.load().mlmc_chebyshev_connection_table(m, _lib.ptr(out), out.size))
    return out.reshape(m, m)


@pytest.fixture(scope="module")
def exact():
    """b = a^-1 as Fractions (a is lower triangular with a positive diagonal): b[m][k], forward substitution row by row."""
    a = _exact_connection(M)                         # a[k][m], m <= k, m = k (mod 2)
    b = [[Fraction(0)] * M for _ in range(M)]
    for m in range(M):
        b[m][m] = 1 / a[m][m]
        # (b a)_mj = delta_mj for j < m:  b_mj a_jj = - sum_{j < k <= m} b_mk a_kj
        for j in range(m - 2, -1, -2):
            acc = sum(b[m][k] * a[k][j] for k in range(j + 2, m + 1, 2))
            b[m][j] = -acc / a[j][j]
    return b


def test_connection_table_against_exact_rationals(exact):
    """Extended precision, rounded once: every entry within one unit in the last place of the exact value, structural zeros exact."""
    t = _lib_connection(M)
    for m in range(M):
        for k in range(M):
            e = exact[m][k]
            if e == 0:
                assert t[m, k] == 0.0, (m, k, t[m, k])
            else:
                ef = float(e)
                assert abs(Fraction(t[m, k]) - e) <= Fraction(np.spacing(abs(ef))), (m, k, t[m, k], ef)
    # a smaller table is the leading block
    assert np.array_equal(_lib_connection(9), t[:9, :9])
    assert np.array_equal(_lib_connection(1), [[1.0]])


def test_connection_table_properties(exact):
    t = _lib_connection(M)
    assert t[0, 0] == 1.0 and not t[0, 1:].any()                       # exact counts / exact zeros: T_0 = P_0
    I, K = np.meshgrid(np.arange(M), np.arange(M), indexing="ij")
    assert not t[(K > I) | ((I - K) % 2 == 1)].any()                   # degree and parity
    assert np.all(np.diag(t) > 0) and np.all(t[K < I] <= 0)
    assert np.count_nonzero(t > 0) == 64 and np.count_nonzero(t < 0) == 992
    assert np.max(np.abs(t.sum(axis=1) - 1.0)) < 8 * np.finfo(float).eps * np.max(np.abs(t).sum(axis=1))   # T_m(1) = P_k(1) = 1
    assert all(sum(row) == 1 for row in exact)
    assert 7.0 < np.max(np.abs(t)) < 7.1 and 13.0 < np.max(np.abs(t).sum(axis=1)) < 13.2
    # T_2 = 4/3 P_2 - 1/3 P_0,  T_3 = 8/5 P_3 - 3/5 P_1
    assert np.array_equal(t[2, :3], [-1 / 3, 0.0, 4 / 3]) and np.array_equal(t[3, :4], [0.0, -0.6, 0.0, 1.6])
    # the change of basis itself
    x = np.array([-1.0, -0.83, -0.1, 0.0, 0.37, 0.99, 1.0])
    P = np.polynomial.legendre.legvander(x, M - 1)
    T = np.polynomial.chebyshev.chebvander(x, M - 1)
    assert np.max(np.abs(P @ t.T - T)) < 2e-14


def test_connection_table_argument_checks():
    from mlmc_amd import _lib
    lib = _lib.load()
    out = np.empty(64 * 64)
    for args in ((0, _lib.ptr(out), out.size), (-3, _lib.ptr(out), out.size), (65, _lib.ptr(out), 65 * 65),
                 (64, _lib.ptr(out), 64 * 64 - 1), (3, _lib.ptr(out), 8), (4, None, 16)):
        assert lib.mlmc_chebyshev_connection_table(*args) != 0
        assert lib.mlmc_last_error().decode() != ""
    assert lib.mlmc_chebyshev_connection_table(3, _lib.ptr(out), 9) == 0


def test_row_sum_route_on_the_benchmark_samples():
    """R = 64, seeded pairs of the benchmark's synthetic workload at its coarsest and finest pair level (steps 0.19 / 0.5 ... and
    0.01 / 0.026).  In double with NumPy (no FMA): the 64 Legendre difference sums by the matrix kernel's scaled monic recurrence,
    turned into the first 64 Chebyshev sums with the exported table; the Chebyshev sums 64..126 by T_k = 2t T_{k-1} - T_{k-2}
    started from the doubling identities as the kernel starts them (TermGen::jump64); contracted with the Chebyshev product
    table.  Reference: Legendre values, products and sums in extended precision.  Gate: 1e-12 of sqrt(sp n), as on the GPU.
    Measured when the route was introduced: 4.4e-16 and 3.5e-16."""
    from oracle import oracle_np as onp
    assert np.finfo(np.longdouble).eps < 2e-19
    R, L, N = 64, 5, 30000
    K1 = 2 * R - 1
    steps = [s[0] for s in onp.determine_level_parameters(L, [0.5, 0.01])]
    shift, scale = DOMAIN[0], 2.0 / (DOMAIN[1] - DOMAIN[0])
    ld = np.longdouble
    b = _lib_connection(M)
    t1 = _lib_table(R, 2)

    def legendre_ld(t, K):
        P = np.empty((K, t.size), dtype=ld)
        tl = t.astype(ld)
        P[0] = 1
        P[1] = tl
        for k in range(2, K):
            P[k] = ((2 * k - 1) * tl * P[k - 1] - (k - 1) * P[k - 2]) / k
        return P

    worst = []
    for l in (1, L - 1):
        f, c = onp.synth_level_samples(l, N, steps)
        tf, tc = (f - shift) * scale + (-1.0), (c - shift) * scale + (-1.0)
        keep = (tf >= -1.0) & (tf <= 1.0) & (tc >= -1.0) & (tc <= 1.0)
        tf, tc = tf[keep], tc[keep]
        n = tf.size
        F, C = legendre_ld(tf, R), legendre_ld(tc, R)
        s_ref = F @ F.T - C @ C.T
        F2, C2, FC = F * F, C * C, F * C
        sp_ref = F2 @ F2.T + C2 @ C2.T - 2 * (FC @ FC.T)
        gate_scale = np.sqrt(np.abs(sp_ref) * n).astype(float) + 1e-300
        S = np.concatenate([b @ cx.legendre_monic_sums(tf, tc, M), cx.chebyshev_sums(tf, tc, K1)[M:]])
        assert S[0] == 0.0
        s = np.tensordot(S, t1, axes=(0, 0))
        assert s[0, 0] == 0.0
        worst.append(float(np.max(np.abs(s - s_ref) / gate_scale)))
    print("means / sqrt(sp n):", worst)
    assert max(worst) < 1e-12, worst
