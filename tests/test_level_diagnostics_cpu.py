"""CPU tests of the level diagnostics: the exported symbols, the long-double reference helper against exact rational
arithmetic, mlmc_diag_merge (host arithmetic), the host statistics of mlmc_amd.diagnostics against SciPy / NumPy, the rates,
the flags, and the route's error without a device."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import level_diag_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_the_abi_version_stays():
    from mlmc_amd import _lib
    lib = _lib.load()
    for name in ("mlmc_level_diagnostics", "mlmc_diag_merge"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    hdr = open(os.path.join(ROOT, "include", "mlmc_hip.h")).read()
    assert int(re.search(r"#define MLMC_ABI_VERSION (\d+)", hdr).group(1)) == 8 == _lib.ABI_VERSION == lib.mlmc_abi_version()
    assert int(re.search(r"#define MLMC_DIAG_NSTAT (\d+)", hdr).group(1)) == 9
    from mlmc_amd import diagnostics
    assert diagnostics.N_STAT == 9 == ref.N_STAT


def _offset_samples(n=4001, seed=5):
    rng = np.random.default_rng(seed)
    return 1e6 + 1e-3 * rng.standard_normal(n), 1e6 + 1e-3 * rng.standard_normal(n)


def _exact(f, c):
    """the nine statistics and their scales in exact rational arithmetic"""
    F = [Fraction(float(v)) for v in f]
    Cc = [Fraction(float(v)) for v in c]
    Y = [Fraction(float(v)) for v in (np.asarray(f) - np.asarray(c))]
    n = len(F)

    def cen(X):
        mean = sum(X) / n
        return mean, [x - mean for x in X]
    my, dy = cen(Y)
    mf, df = cen(F)
    mc, dc = cen(Cc)
    out = [my] + [sum(d ** k for d in dy) for k in (2, 3, 4)] + [mf, sum(d * d for d in df), mc, sum(d * d for d in dc),
                                                                 sum(a * b for a, b in zip(df, dc))]
    scale = [None, out[1], sum(abs(d) ** 3 for d in dy), out[3], None, out[5], None, out[7],
             sum(abs(a) * abs(b) for a, b in zip(df, dc))]
    return out, scale


def test_reference_helper_against_exact_fractions():
    f, c = _offset_samples()
    n, n_rm, got, _ = ref.stats(f, c)
    assert (n, n_rm) == (4001, 0)
    want, scale = _exact(f, c)
    worst = 0.0
    for s in ref.SUM_IDX:
        err = abs(Fraction(float(got[s])) + Fraction(float(got[s] - ref.LD(float(got[s])))) - want[s])
        worst = max(worst, float(err / (scale[s] * Fraction(2) ** -53)))
    for s in ref.MEAN_IDX:
        sd = float(want[s + 1] / n) ** 0.5
        err = abs(Fraction(float(got[s])) + Fraction(float(got[s] - ref.LD(float(got[s])))) - want[s])
        worst = max(worst, float(err) / (2.0 ** -53 * (abs(float(want[s])) + sd)))
    print("reference helper against Fractions: worst %.4f units" % worst)
    assert worst < 0.1


def _merge(lib, a, na, b, nb):
    from mlmc_amd import _lib
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    out = np.zeros(9)
    _lib.check(lib.mlmc_diag_merge(_lib.ptr(a), na, _lib.ptr(b), nb, _lib.ptr(out)))
    return out


def _merge_inputs(kind, n, rng):
    """Inputs with |mean| <= sd.  The merge takes the means of its two sides rounded to fp64; an error of 2^-54 |mean| in one of
    them enters M2 through the term d^2 na nb / n as |d| 2^-53 |mean| na nb / n -- with |mean| = 1e9 sd (the offset inputs of the
    device test) that alone is 1e7 units of 2^-53 sum |x - mean|^2 for ANY arithmetic, so a split of such data cannot be held
    to the gate; with |mean| <= sd it is below one unit and the gate measures the merge itself."""
    z, w = rng.standard_normal(n), rng.standard_normal(n)
    if kind == "normal":
        return z, 0.9 * z + 0.3 * w
    if kind == "lognormal":
        return np.exp(2.0 * z), np.exp(2.0 * (0.9 * z + 0.3 * w))
    return np.sort(z), np.sort(w)                         # sorted: the sides of a split have very different means


@pytest.mark.parametrize("n", [2, 65, 20011])
def test_merge_of_a_split_equals_the_whole(n):
    from mlmc_amd import _lib
    lib = _lib.load()                                     # no device: host arithmetic only
    rng = np.random.default_rng(n)
    worst = [0.0, 0.0]
    for kind in ("normal", "lognormal", "sorted"):
        f, c = _merge_inputs(kind, n, rng)
        for pair in (True, False):
            cc = c if pair else None
            _, _, whole, scale = ref.stats(f, cc)
            for k in sorted({1, max(n // 3, 1), n - 1}):
                na, _, a, _ = ref.stats(f[:k], None if cc is None else cc[:k])
                nb, _, b, _ = ref.stats(f[k:], None if cc is None else cc[k:])
                got = _merge(lib, a.astype(np.float64), na, b.astype(np.float64), nb)
                if not pair:
                    assert np.all(np.isnan(got[6:]))
                um, us = ref.worst_units(got, whole, scale)
                worst = [max(worst[0], um), max(worst[1], us)]
                assert um <= ref.GATE_MEAN and us <= ref.GATE_SUM, (kind, pair, n, k, um, us)
    print("mlmc_diag_merge n = %d: worst mean %.2f units, worst central sum %.2f units" % (n, worst[0], worst[1]))


def test_merge_returns_the_other_side_of_an_empty_one_bit_for_bit():
    from mlmc_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(1)
    a = rng.standard_normal(9)
    a[6:] = np.nan                                        # a level-0 row
    empty = np.full(9, np.nan)
    for got in (_merge(lib, a, 7, empty, 0), _merge(lib, empty, 0, a, 7)):
        assert got.tobytes() == a.tobytes()
    assert np.all(np.isnan(_merge(lib, empty, 0, empty, 0)))
    out = a.copy()                                        # in place
    _lib.check(lib.mlmc_diag_merge(_lib.ptr(out), 7, _lib.ptr(empty), 0, _lib.ptr(out)))
    assert out.tobytes() == a.tobytes()
    # a side with an infinite mean: the union has it (not inf - inf), whichever side it is
    b = rng.standard_normal(9)
    inf_side = b.copy()
    inf_side[[0, 4]] = np.inf
    inf_side[[1, 2, 3, 5, 8]] = np.nan
    for got in (_merge(lib, a, 7, inf_side, 5), _merge(lib, inf_side, 5, a, 7)):
        assert got[0] == np.inf and got[4] == np.inf and np.all(np.isnan(got[[1, 2, 3, 5]]))
    got = _merge(lib, b, 7, inf_side, 5)
    assert np.isfinite(got[6]) and np.isfinite(got[7])
    assert lib.mlmc_diag_merge(None, 1, _lib.ptr(a), 1, _lib.ptr(out)) != 0
    assert b"mlmc_diag_merge" in lib.mlmc_last_error()
    assert lib.mlmc_diag_merge(_lib.ptr(a), -1, _lib.ptr(a), 1, _lib.ptr(out)) != 0


def _stats_of(levels):
    n, _, st, _ = ref.levels_stats(levels)
    return n, st.astype(np.float64)


def test_host_statistics_against_scipy_and_numpy():
    from scipy import stats as sps
    from mlmc_amd import diagnostics
    rng = np.random.default_rng(3)
    L, M, N = 3, 4, [500, 300, 120]
    levels = []
    for l in range(L):
        f = rng.standard_normal((M, N[l])) * (1.0 + np.arange(M))[:, None] + 0.5
        f[1] = np.exp(f[1])                               # a skewed component
        c = None if l == 0 else f + 0.2 * rng.standard_normal((M, N[l])) ** 3
        levels.append((f, c))
    n, st = _stats_of(levels)
    d = diagnostics.from_central_sums(n, st)
    assert d.n_samples.dtype == np.int64 and np.array_equal(d.n_samples, n)
    for name in d.FIELDS:
        assert getattr(d, name).shape == (L, M), name

    def close(a, b):
        return abs(a - b) <= 1e-12 * abs(b)
    for l, (f, c) in enumerate(levels):
        for m in range(M):
            y = f[m] if c is None else f[m] - c[m]
            assert close(d.mean_diff[l, m], np.mean(y)) and close(d.var_diff[l, m], np.var(y, ddof=1))
            assert close(d.skew_diff[l, m], sps.skew(y))
            assert close(d.kurtosis_diff[l, m], sps.kurtosis(y, fisher=False, bias=True))
            assert close(d.mean_fine[l, m], np.mean(f[m])) and close(d.var_fine[l, m], np.var(f[m], ddof=1))
            if c is None:
                for name in ("mean_coarse", "var_coarse", "corr_fine_coarse", "consistency"):
                    assert np.isnan(getattr(d, name)[l, m]), name
            else:
                assert close(d.mean_coarse[l, m], np.mean(c[m])) and close(d.var_coarse[l, m], np.var(c[m], ddof=1))
                assert close(d.corr_fine_coarse[l, m], np.corrcoef(f[m], c[m])[0, 1])
                fp = levels[l - 1][0][m]
                want = abs(np.mean(c[m]) - np.mean(fp)) / (3.0 * (np.sqrt(np.var(c[m], ddof=1) / c[m].size) +
                                                                  np.sqrt(np.var(fp, ddof=1) / fp.size)))
                assert close(d.consistency[l, m], want)
    assert np.allclose(d.mlmc_mean, np.sum(d.mean_diff, axis=0), rtol=1e-15)
    assert np.allclose(d.mlmc_var, np.sum(d.var_diff / n, axis=0), rtol=1e-15)


def test_nan_and_small_counts_never_raise():
    from mlmc_amd import diagnostics
    f0 = np.array([[1.0, 2.0, 4.0], [np.nan, np.nan, np.nan], [np.nan, 5.0, np.nan], [3.0, 3.0, 3.0]])
    f1 = np.array([[1.0, 2.5], [1.0, 2.0], [1.0, np.nan], [3.0, 3.0]])
    c1 = np.array([[0.5, 2.0], [np.nan, np.nan], [0.0, 1.0], [3.0, 3.0]])
    n, st = _stats_of([(f0, None), (f1, c1)])
    assert n.tolist() == [[3, 0, 1, 3], [2, 0, 1, 2]]
    with np.errstate(all="raise"):                        # the module silences its own 0 / 0
        d = diagnostics.from_central_sums(n, st, level_steps=[0.5, 0.1])
        r = d.rates()
        flags = d.flags()
    for name in d.FIELDS[1:]:
        assert np.all(np.isnan(getattr(d, name)[:, 1])), name          # no kept sample
    assert d.mean_diff[0, 2] == 5.0 and d.mean_fine[0, 2] == 5.0 and d.mean_diff[1, 2] == 1.0   # one kept sample: the value
    for name in ("var_diff", "skew_diff", "kurtosis_diff", "var_fine", "consistency"):
        assert np.all(np.isnan(getattr(d, name)[:, 2])), name
    assert np.isnan(d.kurtosis_diff[0, 3]) and d.var_diff[0, 3] == 0.0 and np.isnan(d.corr_fine_coarse[1, 3])   # constant data
    assert np.isfinite(d.consistency[1, 0]) and np.isnan(d.consistency[1, 3])
    assert not flags.any() and flags.dtype == bool and flags.shape == (2, 4)
    assert np.all(np.isnan(r.alpha)) and np.all(np.isnan(r.beta)) and np.isnan(r.gamma) and np.all(np.isnan(r.bias))
    with pytest.raises(ValueError, match=r"\[L, M, 9\]"):
        diagnostics.from_central_sums(n, st[:, :, :8])
    with pytest.raises(ValueError, match="level steps"):
        diagnostics.from_central_sums(n, st, level_steps=[0.5, 0.1, 0.01])


def _hand_made(L=2, M=1):
    n = np.full((L, M), 10, dtype=np.int64)
    st = np.zeros((L, M, 9))
    return n, st


def test_consistency_formula_on_hand_made_numbers():
    from mlmc_amd import diagnostics
    n, st = _hand_made()
    n[0, 0], n[1, 0] = 101, 26
    st[0, 0, 4], st[0, 0, 5] = 2.0, 100.0 * 4.0           # level 0: mean_f = 2, var_f = 4 -> var / n = 4 / 101
    st[1, 0, 6], st[1, 0, 7] = 3.5, 25.0 * 9.0            # level 1: mean_c = 3.5, var_c = 9 -> var / n = 9 / 26
    st[0, 0, 6:] = np.nan
    d = diagnostics.from_central_sums(n, st)
    want = 1.5 / (3.0 * (np.sqrt(9.0 / 26.0) + np.sqrt(4.0 / 101.0)))
    assert np.isnan(d.consistency[0, 0]) and abs(d.consistency[1, 0] - want) <= 1e-15
    assert d.flags(consistency_max=want * 0.999)[1, 0] and not d.flags(consistency_max=want * 1.001)[1, 0]


def _power_law(L):
    from mlmc_amd import diagnostics
    h = 0.5 * 0.25 ** np.arange(L)
    n = np.full((L, 2), 1000, dtype=np.int64)
    st = np.zeros((L, 2, 9))
    st[:, 0, 0] = 3.0 * h                                 # alpha = 1
    st[:, 1, 0] = -0.2 * h                                # a negative mean: |mean|
    st[:, :, 1] = (7.0 * h ** 2 * 999.0)[:, None]         # beta = 2
    st[:, :, 3] = 1.0
    return diagnostics.from_central_sums(n, st, level_steps=h, n_ops=11.0 * h ** -1.5), h


def test_rates_recover_exact_power_laws():
    d, h = _power_law(5)
    r = d.rates()
    assert np.all(np.abs(r.alpha - 1.0) <= 1e-12) and np.all(np.abs(r.beta - 2.0) <= 1e-12) and abs(r.gamma - 1.5) <= 1e-12
    want = np.abs(d.mean_diff[-1]) / (h[-2] / h[-1] - 1.0)
    assert np.all(np.abs(r.bias - want) <= 1e-12 * want)
    # a zero or non-finite entry leaves its level out of that component's fit
    d.mean_diff[2, 0] = 0.0
    d.var_diff[3, 1] = np.nan
    r = d.rates()
    assert np.all(np.abs(r.alpha - 1.0) <= 1e-12) and np.all(np.abs(r.beta - 2.0) <= 1e-12)
    # growing differences: no bias estimate
    d.mean_diff[:, 1] = 1.0 / h
    r = d.rates()
    assert abs(r.alpha[1] + 1.0) <= 1e-12 and np.isnan(r.bias[1]) and np.isfinite(r.bias[0])
    # two levels: one level in the fit
    d2, _ = _power_law(2)
    r2 = d2.rates()
    assert np.all(np.isnan(r2.alpha)) and np.all(np.isnan(r2.beta)) and np.all(np.isnan(r2.bias))
    assert abs(r2.gamma - 1.5) <= 1e-12
    d2.n_ops = None
    assert np.isnan(d2.rates().gamma)


def test_flags():
    from mlmc_amd import diagnostics
    n, st = _hand_made(L=2, M=3)
    st[:, :, 1] = 10.0                                    # m2 = 1
    st[:, :, 3] = 10.0 * np.array([[3.0, 100.0, 100.5], [np.nan, 250.0, 2.0]])      # kurtosis
    st[:, :, 5] = st[:, :, 7] = 90.0                      # var_f = var_c = 10 -> standard errors 1
    st[1, :, 6] = [5.9, 0.0, 6.1]                         # consistency 5.9 / 6, 0, 6.1 / 6
    d = diagnostics.from_central_sums(n, st)
    assert d.flags().tolist() == [[False, False, True], [False, True, True]]
    assert d.flags(kurtosis_max=2.5, consistency_max=0.5).tolist() == [[True, True, True], [True, True, True]]
    assert d.flags(kurtosis_max=1e3, consistency_max=2.0).tolist() == [[False] * 3] * 2


def test_estimate_level_diagnostics_raises_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mlmc_amd import _lib
    from mlmc_amd.estimator import Estimate
    from tests.test_component_moments_cpu import _estimate
    est, _ = _estimate()
    with pytest.raises(_lib.MlmcHipError):
        est.estimate_level_diagnostics()
    assert isinstance(est, Estimate)
