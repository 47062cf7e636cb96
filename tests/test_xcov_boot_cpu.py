"""CPU checks of the component-covariance bootstrap: the long-double reference of tests/xcov_boot_cases.py against exact rational
arithmetic, the calibration of the fp64 twins (printed with pytest -s, pinned by XCOV_BOOT_TWIN_UNITS, from which
tests/test_gpu_xcov_boot.py derives the device tolerances), deliberately broken twins that the tolerances must catch, the host
finish (estimator.covariance_replicates), the argument errors raised before any device work, the ABI, and a seeded statistical check
of the finish under NumPy's multinomial weights."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import xcov_boot_cases as xc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the reference against exact rational arithmetic ----------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("shift", [None, (2, -1, 3)])
def test_reference_equals_rational_arithmetic(pair, shift):
    rng = np.random.default_rng(11 + int(pair))
    M, n = 3, 41
    f = rng.integers(-6, 7, size=(M, n)).astype(np.float64)
    c = rng.integers(-6, 7, size=(M, n)).astype(np.float64) if pair else None
    f[1, 4] = np.nan
    if pair:
        c[2, 9] = np.nan
    w = rng.integers(0, 4, size=(2, n))
    cnt, s1, s2, U1, U2 = xc.weighted_sums(f, c, shift, w)
    a = [Fraction(0)] * M if shift is None else [Fraction(v) for v in shift]
    for b in range(2):
        n_x = 0
        x1 = [Fraction(0)] * M
        x2 = [[Fraction(0)] * M for _ in range(M)]
        for k in range(n):
            if np.isnan(f[:, k]).any() or (pair and np.isnan(c[:, k]).any()):
                continue
            ft = [Fraction(int(f[m, k])) - a[m] for m in range(M)]
            ct = [Fraction(int(c[m, k])) - a[m] for m in range(M)] if pair else [Fraction(0)] * M
            wk = int(w[b, k])
            n_x += wk
            for i in range(M):
                x1[i] += wk * (ft[i] - ct[i])
                for j in range(M):
                    x2[i][j] += wk * (ft[i] * ft[j] - ct[i] * ct[j])
        assert cnt[b] == n_x
        for i in range(M):
            assert Fraction(int(s1[b, i])) == x1[i] and float(s1[b, i]) == float(x1[i])
            for j in range(M):
                assert Fraction(int(s2[b, i, j])) == x2[i][j] and float(s2[b, i, j]) == float(x2[i][j])
    assert np.array_equal(s2, s2.transpose(0, 2, 1))
    assert np.all(U1 >= np.abs(s1)) and np.all(U2 >= np.abs(s2))


# ---- 2. the twins: calibration and what the tolerance catches ----------------------------------------------------------------------
def _calibration_runs():
    for name, M, n, offset in xc.CALIBRATION:
        for pair in (False, True):
            for kind in ("zero", "mean"):
                f, c = xc.make_chunk(M, n, 1, pair, offset)
                shift = xc.make_shift(M, kind, offset)
                w = xc.multinomial_weights(n, xc.calibration_sizes(n), M)
                yield "{}/{}/{}".format(name, "pair" if pair else "level0", kind), "pair" if pair else "level0", f, c, shift, w


@pytest.fixture(scope="module")
def calibration():
    table = {cls: {q: [0.0, 0.0] for q in xc.QUANTITIES} for cls in xc.CLASSES}
    where = {}
    runs = []
    for tag, cls, f, c, shift, w in _calibration_runs():
        ref = xc.weighted_sums(f, c, shift, w)
        runs.append((tag, cls, f, c, shift, w, ref))
        for t, variant in enumerate("AB"):
            got = xc.weighted_sums(f, c, shift, w, np.float64, variant)
            assert np.array_equal(got[0], ref[0])
            for q, g, r, s in (("s1", got[1], ref[1], ref[3]), ("s2", got[2], ref[2], ref[4])):
                u = xc.units(g, r, s)
                if u > table[cls][q][t]:
                    table[cls][q][t] = u
                    where[cls, q, t] = tag
    return table, where, runs


def _two_digits(measured, recorded):
    return abs(measured - recorded) <= 0.006 * max(recorded, 1.0) + 0.05


def test_twin_calibration_table(calibration):
    """both twins on every calibration case: the worst units per class are the recorded XCOV_BOOT_TWIN_UNITS to two digits"""
    table, where, _ = calibration
    print()
    for cls in table:
        for q, (a, b) in table[cls].items():
            print("twin units {:7s} {:3s}  A {:9.4g} ({})  B {:9.4g} ({})  -> device tolerance {:g} units".format(
                cls, q, a, where.get((cls, q, 0)), b, where.get((cls, q, 1)), max(16.0, 4 * max(a, b))))
    assert set(table) == set(xc.XCOV_BOOT_TWIN_UNITS)
    for cls in table:
        assert set(table[cls]) == set(xc.XCOV_BOOT_TWIN_UNITS[cls])
        for q, (a, b) in table[cls].items():
            ra, rb = xc.XCOV_BOOT_TWIN_UNITS[cls][q]
            assert _two_digits(a, ra) and _two_digits(b, rb), (cls, q, a, b, ra, rb)
            assert xc.tolerance(cls, q) == max(16.0, 4.0 * max(ra, rb))


@pytest.mark.parametrize("flaw", ["no_coarse", "keep_nan", "coarse_unshifted"])
def test_the_tolerance_catches_a_broken_twin(calibration, flaw):
    """a dropped coarse term, a sample kept despite a NaN, a forgotten shift on the coarse side: each is far outside the tolerance
    (or changes a count) on a pair-level case with a non-zero shift"""
    _, _, runs = calibration
    tag, cls, f, c, shift, w, ref = next(r for r in runs if r[0] == "M5_n4097/pair/mean")
    got = xc.weighted_sums(f, c, shift, w, np.float64, "B", flaw=flaw)
    u1, u2 = xc.units(got[1], ref[1], ref[3]), xc.units(got[2], ref[2], ref[4])
    print("\n{}: s1 {:.3g} units, s2 {:.3g} units, counts equal: {}".format(flaw, u1, u2, np.array_equal(got[0], ref[0])))
    assert max(u1 / xc.tolerance(cls, "s1"), u2 / xc.tolerance(cls, "s2")) > 1e3
    if flaw == "keep_nan":
        assert not np.array_equal(got[0], ref[0])


# ---- 3. the host finish ----------------------------------------------------------------------------------------------------------------
def _unit_weight_sums(x, shift=None):
    """n, s1, s2 [1, 1, ...] of weights all equal to 1 on one level"""
    a = np.zeros(x.shape[0]) if shift is None else np.asarray(shift)
    xt = x - a[:, None]
    return np.array([[x.shape[1]]]), xt.sum(axis=1)[None, None], (xt @ xt.T)[None, None]


def test_finish_reproduces_numpy_cov_and_corrcoef():
    from mlmc_amd.estimator import covariance_replicates
    rng = np.random.default_rng(5)
    x = rng.normal(size=(4, 300)) + np.array([[3.0], [0.0], [-2.0], [10.0]])
    x[1] += 0.7 * x[0]
    for shift in (None, x.mean(axis=1) + 0.01):
        n, s1, s2 = _unit_weight_sums(x, shift)
        mean, cov, corr, ok = covariance_replicates(n, s1, s2, [300], shift)
        assert ok.tolist() == [True]
        assert np.allclose(mean[0], x.mean(axis=1), rtol=0, atol=1e-13)
        assert np.allclose(cov[0], np.cov(x, bias=True), rtol=0, atol=1e-13)
        assert np.allclose(corr[0], np.corrcoef(x), rtol=0, atol=1e-13)
        assert np.array_equal(cov[0], cov[0].T) and np.array_equal(corr[0], corr[0].T) and np.all(np.diag(corr[0]) == 1.0)
    n, s1, s2 = _unit_weight_sums(x)
    raw = covariance_replicates(n, s1, s2, [300], None, centered=False)[1]
    assert np.allclose(raw[0], x @ x.T / 300, rtol=1e-14) and np.array_equal(raw[0], raw[0].T)


def test_finish_skips_levels_without_requested_samples_and_flags_bad_replicates():
    from mlmc_amd.estimator import covariance_replicates
    rng = np.random.default_rng(6)
    x0, x1 = rng.normal(size=(2, 50)), rng.normal(size=(2, 20))
    a0, a1 = _unit_weight_sums(x0), _unit_weight_sums(x1)
    n = np.concatenate([a0[0], a1[0]], axis=1)
    s1 = np.concatenate([a0[1], a1[1]], axis=1)
    s2 = np.concatenate([a0[2], a1[2]], axis=1)
    both = covariance_replicates(n, s1, s2, [50, 20])
    only0 = covariance_replicates(n, s1, s2, [50, 0])
    alone = covariance_replicates(*a0, [50])
    assert both[3].all() and only0[3].all()
    for u, v in zip(only0[:3], alone[:3]):
        assert np.array_equal(u, v)
    assert not np.array_equal(both[1], only0[1])
    # a skipped level may hold n = 0 (and NaN sums) without harm; a used level with n = 0 is not ok
    n0 = n.copy()
    n0[0, 1] = 0
    s1n = s1.copy()
    s1n[0, 1] = np.nan
    assert np.array_equal(covariance_replicates(n0, s1n, s2, [50, 0])[1], only0[1])
    mean, cov, corr, ok = covariance_replicates(n0, s1, s2, [50, 20])
    assert ok.tolist() == [False] and np.isnan(mean).all() and np.isnan(cov).all() and np.isnan(corr).all()
    # two replicates, the second with a constant component: its variance is zero
    y = x0.copy()
    y[1] = 4.0
    b0, b1 = _unit_weight_sums(x0), _unit_weight_sums(y)
    mean, cov, corr, ok = covariance_replicates(*(np.concatenate(p, axis=0) for p in zip(b0, b1)), [50])
    assert ok.tolist() == [True, False]
    assert np.isfinite(cov[0]).all() and np.isnan(cov[1]).all() and np.isnan(corr[1]).all() and np.isnan(mean[1]).all()
    with pytest.raises(ValueError):
        covariance_replicates(n, s1, s2[:, :, :1], [50, 20])
    with pytest.raises(ValueError):
        covariance_replicates(n, s1, s2, [50])


# ---- 4. argument errors before any device work ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def estimate():
    from mlmc_amd.estimator import Estimate
    from tests.test_gpu_bootstrap_batch import _levels, _memory, _root_q
    st = _memory(_levels([60, 30], 3, nan=False), 3)
    return Estimate(_root_q(st, 3), st)


def test_argument_errors_come_before_device_work(estimate):
    e = estimate
    eye = np.eye(3)
    for call in (lambda: e.est_bootstrap_component_covariance(4, corr=eye),
                 lambda: e.bootstrap_component_correlation(4, corr=eye),
                 lambda: e.bootstrap_joint_probability(-1.0, 1.0, 4, corr=eye),
                 lambda: e.bootstrap_joint_exceedance(0.0, 4, corr=eye)):
        with pytest.raises(ValueError, match="nothing to resample"):
            call()
    with pytest.raises(ValueError, match="corr must be None or 'scores'"):
        e.est_bootstrap_component_covariance(4, corr="pearson")
    with pytest.raises(ValueError, match="marginals must be 'fixed' or 'resampled'"):
        e.bootstrap_joint_probability(-1.0, 1.0, 4, marginals="both")
    with pytest.raises(ValueError, match="marginals"):
        e.bootstrap_joint_exceedance(0.0, 4, marginals=None)
    for level in (0.0, 1.0, True, "0.9"):
        with pytest.raises(ValueError, match="level must be a number in"):
            e.bootstrap_component_correlation(4, level=level)
        with pytest.raises(ValueError, match="level must be a number in"):
            e.bootstrap_joint_probability(-1.0, 1.0, 4, level=level)
    for k in ([61, 30], [10, -1], [1.5, 3], [10]):
        with pytest.raises(ValueError, match="sample_vector"):
            e.est_bootstrap_component_covariance(4, sample_vector=k)
        with pytest.raises(ValueError, match="sample_vector"):
            e.bootstrap_component_correlation(4, sample_vector=k)
        with pytest.raises(ValueError, match="sample_vector"):
            e.bootstrap_joint_exceedance(0.0, 4, sample_vector=k)
    with pytest.raises(ValueError, match="n_subsamples"):
        e.est_bootstrap_component_covariance(0)
    with pytest.raises(ValueError, match="seed"):
        e.est_bootstrap_component_covariance(4, seed=-1)
    with pytest.raises(ValueError, match="NaN"):
        e.bootstrap_joint_exceedance([0.0, np.nan, 0.0], 4)
    with pytest.raises(ValueError, match="at least one seed"):
        e.bootstrap_joint_probability(-1.0, 1.0, 4, seeds=())


def test_scores_and_shift_exclude_each_other(estimate):
    from mlmc_amd.quantity import quantity_estimate as qe
    q = estimate.quantity
    with pytest.raises(ValueError, match="scores and shift exclude each other"):
        qe.bootstrap_component_covariance(q, 4, [60, 30], 1, shift=np.zeros(3), scores=[object()] * 3)
    with pytest.raises(ValueError, match="2 score distributions for 3 components"):
        qe.bootstrap_component_covariance(q, 4, [60, 30], 1, scores=[object()] * 2)
    with pytest.raises(ValueError, match="shift of shape"):
        qe.bootstrap_component_covariance(q, 4, [60, 30], 1, shift=np.zeros(2))
    with pytest.raises(ValueError, match="finite"):
        qe.bootstrap_component_covariance(q, 4, [60, 30], 1, shift=[0.0, np.inf, 0.0])
    with pytest.raises(TypeError):
        qe.bootstrap_component_covariance(qe.component_covariance(q), 4, [60, 30], 1)


# ---- 5. the ABI --------------------------------------------------------------------------------------------------------------------------
def test_abi_exports_the_three_entries_within_version_8():
    from mlmc_amd import _lib
    names = ("mlmc_bootstrap_create_xcov", "mlmc_bootstrap_set_shift", "mlmc_bootstrap_finalize_xcov")
    header = open(os.path.join(ROOT, "include", "mlmc_hip.h")).read()
    assert re.search(r"#define MLMC_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8
    comment = header[header.index("#define MLMC_ABI_VERSION"):header.index("/* basis kinds")]
    lib = _lib.load()
    assert lib.mlmc_abi_version() == 8
    for name in names:
        assert name in comment, name                              # named in the version comment
        assert re.search(r"\bint {}\(".format(name), header), name
        assert name in _lib.SIGNATURES
        getattr(lib, name)                                        # exported


# ---- 6. a seeded statistical check of the finish --------------------------------------------------------------------------------------
def test_spread_of_the_replicate_correlations_matches_the_asymptotic_law():
    """bivariate normal, rho = 0.6, n = 4000 on one level, B = 400 NumPy multinomial resamples of size n: the standard deviation of
    the replicate correlations over (1 - rho^2) / sqrt(n) lies in [0.8, 1.25] (the noise of a standard deviation from 400
    replicates is 1 / sqrt(2 B) = 3.5 %)."""
    from mlmc_amd.estimator import covariance_replicates
    rho, n, B = 0.6, 4000, 400
    rng = np.random.default_rng(2024)
    z = rng.normal(size=(2, n))
    x = np.stack([z[0], rho * z[0] + np.sqrt(1.0 - rho * rho) * z[1]])
    w = rng.multinomial(n, np.full(n, 1.0 / n), size=B).astype(np.float64)
    a = x.mean(axis=1)
    xt = x - a[:, None]
    cnt = w.sum(axis=1).astype(np.int64)[:, None]
    s1 = (w @ xt.T)[:, None, :]
    s2 = np.einsum("bk,ik,jk->bij", w, xt, xt)[:, None]
    mean, cov, corr, ok = covariance_replicates(cnt, s1, s2, [n], a)
    assert ok.all() and np.all(cnt == n)
    ratio = np.std(corr[:, 0, 1], ddof=1) / ((1.0 - rho * rho) / np.sqrt(n))
    print("\nstd of the replicate correlations / asymptotic value:", ratio, " mean:", corr[:, 0, 1].mean(), " data:", np.corrcoef(x)[0, 1])
    assert 0.8 <= ratio <= 1.25, ratio
    assert abs(corr[:, 0, 1].mean() - np.corrcoef(x)[0, 1]) < 3 * (1.0 - rho * rho) / np.sqrt(n)
