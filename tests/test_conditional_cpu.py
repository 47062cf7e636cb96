"""CPU tests of conditioning under the Gaussian copula: the host side of tool.simple_distribution (conditional_factor, the parsing of
`given`, the argument checks of conditional_samples) against the long-double Schur complement of tests/conditional_cases.py, the
host map p -> Phi(mu + s Phi^-1(p)) against mpmath, and the NumPy restatement of the statistics that
tests/test_gpu_conditional_samples.py asks of the device's draws."""
import itertools
import os
import re

import numpy as np
import pytest
from scipy import special

from tests import conditional_cases as cc
from tests import joint_sample_cases as jc
from tests import sample_cases as sc

SEED = 0x9E3779B97F4A7C15                            # of the sampling tests
FAR = 2 ** 33 + 1
NAME = "mlmc_density_sample_conditional_batch"


def _sd():
    from mlmc_amd.tool import simple_distribution as sd
    return sd


def _subsets(M, sizes):
    return [o for p in sizes for o in itertools.combinations(range(M), p)]


CORR12 = cc.random_corr(np.random.default_rng(12), 12)
FACTOR_CASES = [(jc.CORR3, o) for o in _subsets(3, (0, 1, 2))] \
    + [(CORR12, tuple(sorted(np.random.default_rng(100 + p).permutation(12)[:p].tolist()))) for p in (1, 5, 11)]


@pytest.mark.parametrize("corr,observed", FACTOR_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"M{len(v)}")
def test_factor_against_the_schur_complement(corr, observed):
    """F_c F_c^T and W against the long-double Schur complement of C' = F F^T within 1e-12; shapes, the triangle, the unit-norm
    identity |L_UO[m]|^2 + s_m^2 = 1 within 1e-14"""
    sd = _sd()
    M, p = corr.shape[0], len(observed)
    w, fc, info = sd.conditional_factor(corr, list(reversed(observed)))             # any order
    assert type(info).__name__ == "ConditionalFactorInfo" and info._fields == ("unobserved", "s", "min_eig_in", "repaired")
    assert w.shape == (M - p, p) and fc.shape == (M - p, M - p) and fc.flags.c_contiguous and fc.dtype == np.float64
    assert np.array_equal(fc, np.tril(fc)) and np.all(np.diag(fc) > 0)
    F, finfo = sd.correlation_factor(corr)
    want_w, want_s, unobs = cc.schur(cc.used_correlation(F), observed)
    assert np.array_equal(info.unobserved, unobs) and info.min_eig_in == finfo.min_eig_in and info.repaired == finfo.repaired
    err_s = float(np.max(np.abs(fc.astype(cc.LD) @ fc.T.astype(cc.LD) - want_s)))
    err_w = float(np.max(np.abs(w - want_w))) if p else 0.0
    print(f"\nM {M} observed {observed}: F_c F_c^T {err_s:.3g}, W {err_w:.3g}")
    assert err_s <= 1e-12 and err_w <= 1e-12
    assert np.all((info.s > 0) & (info.s <= 1.0 + 4 * cc.U)) and np.array_equal(info.s, np.sqrt(np.sum(fc * fc, axis=1)))
    if p == 0:
        assert w.shape == (M, 0) and np.array_equal(fc, F)
    else:
        # L_UO = W L_OO: the part of a row's unit norm that the observed scores explain
        perm = list(observed) + list(unobs)
        low = np.linalg.cholesky((F @ F.T)[np.ix_(perm, perm)])
        assert np.max(np.abs(np.sum(low[p:, :p] ** 2, axis=1) + info.s ** 2 - 1.0)) <= 1e-14


def test_bivariate_closed_form():
    """M = 2: mu = rho z, s^2 = 1 - rho^2"""
    for rho in (0.0, 0.3, -0.8, 0.999):
        corr = np.array([[1.0, rho], [rho, 1.0]])
        for o in (0, 1):
            w, fc, info = _sd().conditional_factor(corr, [o])
            assert w.shape == (1, 1) and abs(w[0, 0] - rho) <= 4 * cc.U and abs(fc[0, 0] ** 2 - (1 - rho * rho)) <= 8 * cc.U
            assert info.unobserved.tolist() == [1 - o] and abs(info.s[0] - np.sqrt(1 - rho * rho)) <= 8 * cc.U / np.sqrt(1 - rho * rho)
            assert abs(float(cc.conditional_mean(w, [[1.7]])[0, 0]) - rho * 1.7) <= 8 * cc.U


def test_indefinite_matrix_is_repaired_as_by_correlation_factor():
    sd = _sd()
    corr = np.array([[1.0, 0.9, 0.9], [0.9, 1.0, -0.9], [0.9, -0.9, 1.0]])
    for min_eig in (1e-10, 1e-3):
        F, finfo = sd.correlation_factor(corr, min_eig=min_eig)
        w, fc, info = sd.conditional_factor(corr, [1], min_eig=min_eig)
        assert info.repaired and finfo.repaired and info.min_eig_in == finfo.min_eig_in == pytest.approx(-0.8, abs=1e-12)
        want_w, want_s, _ = cc.schur(cc.used_correlation(F), [1])
        # the repaired matrix is close to singular (smallest eigenvalue min_eig): the Schur complement loses 1 / min_eig
        assert np.max(np.abs(fc @ fc.T - want_s)) <= 1e-14 / min_eig and np.max(np.abs(w - want_w)) <= 1e-14 / min_eig
        _, fc0, _ = sd.conditional_factor(corr, [], min_eig=min_eig)
        assert np.array_equal(fc0, F)


def test_factor_errors():
    sd = _sd()
    with pytest.raises(ValueError, match="distinct"):
        sd.conditional_factor(jc.CORR3, [1, 1])
    for bad in ([3], [-1], [0, 7]):
        with pytest.raises(ValueError, match="out of range"):
            sd.conditional_factor(jc.CORR3, bad)
    with pytest.raises(ValueError, match="every component is observed"):
        sd.conditional_factor(jc.CORR3, [2, 0, 1])
    for bad in ([0.5], [True], ["a"]):
        with pytest.raises(ValueError, match="component indices"):
            sd.conditional_factor(jc.CORR3, bad)
    with pytest.raises(ValueError, match="square"):
        sd.conditional_factor(np.ones((2, 3)), [0])
    with pytest.raises(ValueError, match="unit diagonal"):
        sd.conditional_factor(2 * np.eye(3), [0])


def test_given_parsing():
    sd = _sd()
    obs, vals, scalar = sd._parse_given("f", {2: 0.5, 0: -1.0}, 4)
    assert obs.tolist() == [0, 2] and vals.tolist() == [[-1.0], [0.5]] and scalar
    obs, vals, scalar = sd._parse_given("f", {2: [0.5, 0.6, 0.7], 0: -1.0, np.int64(3): np.array([1.0, 2.0, 3.0])}, 4)
    assert obs.tolist() == [0, 2, 3] and not scalar
    assert vals.tolist() == [[-1.0] * 3, [0.5, 0.6, 0.7], [1.0, 2.0, 3.0]]                   # a scalar holds in every set
    obs, vals, scalar = sd._parse_given("f", {1: [0.5]}, 2)
    assert vals.shape == (1, 1) and not scalar                                           # an array of one set is an array
    obs, vals, scalar = sd._parse_given("f", {}, 3)
    assert obs.size == 0 and vals.shape == (0, 1) and scalar
    with pytest.raises(ValueError, match="share one length"):
        sd._parse_given("f", {0: [1.0, 2.0], 1: [1.0, 2.0, 3.0]}, 4)
    with pytest.raises(ValueError, match="names component 4"):
        sd._parse_given("f", {4: 1.0}, 4)
    with pytest.raises(ValueError, match="names component -1"):
        sd._parse_given("f", {-1: 1.0}, 4)
    with pytest.raises(ValueError, match="component index"):
        sd._parse_given("f", {0.5: 1.0}, 4)
    with pytest.raises(ValueError, match="every component is given"):
        sd._parse_given("f", {0: 1.0, 1: 2.0}, 2)
    with pytest.raises(ValueError, match="scalar or a 1-D array"):
        sd._parse_given("f", {0: np.ones((2, 2))}, 4)
    with pytest.raises(ValueError, match="are empty"):
        sd._parse_given("f", {0: []}, 4)
    with pytest.raises(ValueError, match="must map"):
        sd._parse_given("f", [0, 1], 4)


def test_conditional_samples_argument_errors():
    """checked before anything touches the device"""
    sd = _sd()
    three = [object()] * 3
    for seed in (None, -1, 2 ** 64, 1.5, True):
        with pytest.raises(ValueError, match="seed"):
            sd.conditional_samples(three, 10, seed, {0: 1.0}, corr=jc.CORR3)
    with pytest.raises(ValueError, match="n must be"):
        sd.conditional_samples(three, -1, 1, {0: 1.0}, corr=jc.CORR3)
    with pytest.raises(ValueError, match="names component 3"):
        sd.conditional_samples(three, 10, 1, {3: 1.0}, corr=jc.CORR3)
    with pytest.raises(ValueError, match="every component is given"):
        sd.conditional_samples(three, 10, 1, {0: 1.0, 1: 1.0, 2: 1.0}, corr=jc.CORR3)
    with pytest.raises(ValueError, match="share one length"):
        sd.conditional_samples(three, 10, 1, {0: [1.0, 2.0], 1: [1.0]}, corr=jc.CORR3)
    for fn in (sd.conditional_quantiles, sd.conditional_cdfs):
        with pytest.raises(ValueError, match="names component 5"):
            fn(three, [0.5], {5: 1.0}, jc.CORR3)


def test_entry_is_declared():
    from mlmc_amd import _lib
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "include", "mlmc_hip.h")).read()
    assert NAME in text.split("#define MLMC_ABI_VERSION")[1].split("*/")[0]
    assert re.search(r"#define\s+MLMC_ABI_VERSION\s+8\b", text) and _lib.ABI_VERSION == 8
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 25
    assert hasattr(_lib.load(), NAME)


def test_probability_map_against_mpmath():
    """p' = ndtr(mu + s ndtri(p)) as conditional_quantiles maps it, against mpmath at 50 digits, in units of 2^-53 max(p', 2^-53)"""
    worst, where = 0.0, None
    for mu in cc.MAP_MU:
        for s in cc.MAP_S:
            got = special.ndtr(mu + s * special.ndtri(cc.MAP_P))
            units = cc.map_units(got, cc.mp_map(cc.MAP_P, mu, s))
            k = int(np.argmax(units))
            if units[k] > worst:
                worst, where = float(units[k]), (mu, s, float(cc.MAP_P[k]))
    print(f"\np -> p' against mpmath: worst {worst:.4g} units at (mu, s, p) = {where} (recorded {cc.MAP_UNITS_OBSERVED}, "
          f"tolerance {jc.tolerance(cc.MAP_UNITS_OBSERVED):g})")
    assert worst <= jc.tolerance(cc.MAP_UNITS_OBSERVED)
    # the ends and what is no probability
    with np.errstate(invalid="ignore"):
        ends = special.ndtr(0.3 + 0.6 * special.ndtri(np.array([0.0, 1.0, np.nan, -0.1, 1.1])))
    assert ends[0] == 0.0 and ends[1] == 1.0 and np.all(np.isnan(ends[2:]))


@pytest.mark.parametrize("first", [0, FAR])
def test_restatement_statistics(first):
    """n = 16384 conditional scores mu + F_c z of the 3 x 3 case from the restated normals, for the observed sets and scores of the
    GPU test: mean, variance and conditional correlation within 5 standard errors, Kolmogorov distance of Phi((y - mu) / s)
    within the DKW bound.  The caps are conditions; the figures are printed so that the margin shows without a GPU."""
    worst = np.zeros(4)
    for observed, z_obs in cc.STAT_CASES:
        w, fc, info = _sd().conditional_factor(jc.CORR3, observed)
        mu = w @ np.array(z_obs)
        z = jc.normals(SEED, range(fc.shape[1]), first, sc.DKW_N)
        y = mu[:, None] + fc @ z
        # what the device does with them and the test undoes: u = Phi(y), score = ndtri(u)
        stats = np.array(cc.score_statistics(special.ndtri(special.ndtr(y)), mu, fc))
        worst = np.maximum(worst, stats)
        assert np.all(stats[:3] <= 5.0) and stats[3] <= sc.DKW_BOUND, (observed, stats)
    print(f"\nfirst = {first}: mean {worst[0]:.3g}, variance {worst[1]:.3g}, correlation {worst[2]:.3g} standard errors, "
          f"Kolmogorov distance {worst[3]:.4f} (bound {sc.DKW_BOUND:.5f})")
