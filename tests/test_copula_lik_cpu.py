"""CPU tests of the copula log-likelihood: the twins of tests/copula_lik_cases.py against their references, the host statistics, the
argument checks that come before any device call, and the two C-ABI entries in header, binding and library."""
import os
import re

import mpmath
import numpy as np
import pytest

from mlmc_amd import estimator
from mlmc_amd.tool import simple_distribution as sd
from tests import copula_lik_cases as lc
from tests import t_copula_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"mlmc_student_t_quantile": 5, "mlmc_copula_log_density": 16}


# ---- the t quantile ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def quantile_table():
    """per nu: the twin's quantiles at p_arguments, their errors in q_units against mpmath, and the trips"""
    rows = []
    for dof in lc.DOFS:
        C, trips = tc.Constants(dof), lc.Trips()
        p = lc.p_arguments()
        y = np.array([lc.twin_t_quantile(C, float(v), trips) for v in p])
        ref = [lc.mp_t_quantile(dof, v, s) for v, s in zip(p, y)]
        units = np.array([lc.q_units(a, r, v, dof) for a, r, v in zip(y, ref, p)])
        rows.append(dict(dof=dof, p=p, y=y, ref=ref, units=units, trips=trips))
    return rows


def test_twin_quantile_against_mpmath(quantile_table):
    print("\n  nu | q units (at p)          | Halley trips")
    for r in quantile_table:
        i = int(np.argmax(r["units"]))
        print("{:4g} | {:8.2f} ({:12.5g}) | {}".format(r["dof"], r["units"][i], r["p"][i], r["trips"].t_newton))
    worst = max(float(np.max(r["units"])) for r in quantile_table)
    assert worst <= lc.Q_UNITS_OBSERVED_TWIN
    assert worst >= 0.9 * lc.Q_UNITS_OBSERVED_TWIN               # the record is the figure of this file's arguments, not a loose bound


def test_twin_quantile_trips_stay_within_half_the_cap(quantile_table):
    for r in quantile_table:
        t = r["trips"]
        assert t.capped == 0 and 2 * t.t_newton <= lc.T_NEWTON_CAP, r["dof"]
        assert t.t_series < tc.T_SERIES_CAP and t.t_lentz < tc.T_LENTZ_CAP


def test_twin_quantile_properties():
    for dof in lc.DOFS:
        C, trips = tc.Constants(dof), lc.Trips()
        assert lc.twin_t_quantile(C, 0.0, trips) == -np.inf and lc.twin_t_quantile(C, 1.0, trips) == np.inf
        assert lc.twin_t_quantile(C, 0.5, trips) == 0.0
        assert all(np.isnan(lc.twin_t_quantile(C, v, trips)) for v in (np.nan, -0.1, 1.5))
        p = np.arange(1, 512, 37) * 2.0 ** -10
        y = np.array([lc.twin_t_quantile(C, float(v), trips) for v in p])
        assert np.all(np.diff(y) > 0.0) and np.all(y < 0.0)
        assert np.array_equal(np.array([lc.twin_t_quantile(C, float(1.0 - v), trips) for v in p]), -y)
        back = np.array([tc.twin_t_cdf(C, float(v), trips) for v in y])
        assert np.max(np.abs(back - p) / p) < 1e-13


# ---- the log density -----------------------------------------------------------------------------------------------------------

def _scores(M, n, dof, seed):
    """scores with heavy tails: t variates of 2 degrees of freedom whatever the model, a few of them extreme"""
    rng = np.random.default_rng([seed, M, n])
    y = rng.standard_t(2.0, size=(M, n))
    y[rng.integers(M), 0] = 1e6 if dof != np.inf else 8.0
    return y


DEFINITION_CASES = [(M, dof) for M in (1, 2, 5, 12) for dof in (1.0, 3.0, 64.0, np.inf)]


def test_long_double_reference_against_the_definition():
    worst = 0.0
    for M, dof in DEFINITION_CASES:
        for g in (0, 1):
            A, _ = lc.inverse_factor(np.ones((1, 1)) if M == 1 else lc.correlation(M, g))
            # the logdet of the model that this fp64 A defines, rounded once
            logdet = float(-np.sum(np.log(np.diag(A).astype(np.longdouble))))
            y = _scores(M, 3, dof, 5)
            ref, scale = lc.long_double_log_density(A, logdet, dof, y)
            for j in range(y.shape[1]):
                want = lc.mp_log_density(A, dof, y[:, j])
                with mpmath.workdps(lc.MP_DIGITS):
                    err = float(abs(mpmath.mpf(float(ref[j])) + mpmath.mpf(float(ref[j] - np.longdouble(float(ref[j])))) - want))
                units = err / (lc.U * scale[j]) if scale[j] > 0 else (0.0 if err == 0.0 else np.inf)
                worst = max(worst, units)
                assert units <= 1.0, (M, dof, g, j, units)
    print("\nlong double against the definition: at most {:.3f} l_units".format(worst))


@pytest.fixture(scope="module")
def twin_density_units():
    """the twin of the chain against the long-double reference on the problems of the GPU tests, scores from SciPy"""
    from scipy import special
    rows = []
    for shape in lc.SHAPES:
        pr = lc.Problem(*shape)
        u = lc.clamp(pr.u_fine[:, :pr.n][:, pr.keep])
        for g in range(pr.G):
            dof = pr.dofs[g]
            y = special.ndtri(u) if dof == np.inf else special.stdtrit(dof, u)
            l = lc.twin_log_density(pr.A[g], pr.logdet[g], dof, y)
            ref, scale = lc.long_double_log_density(pr.A[g], pr.logdet[g], dof, y)
            rows.append((repr(pr), dof, float(np.max(lc.l_units(l, ref, scale))) if y.shape[1] else 0.0))
    return rows


def test_twin_log_density_against_long_double(twin_density_units):
    worst = max(twin_density_units, key=lambda r: r[2])
    print("\nthe twin's largest error: {:.3f} l_units ({}, nu = {:g})".format(worst[2], worst[0], worst[1]))
    assert worst[2] <= lc.L_UNITS_OBSERVED_TWIN
    assert worst[2] >= 0.9 * lc.L_UNITS_OBSERVED_TWIN


def test_the_two_exact_zeros_on_the_twin():
    rng = np.random.default_rng(3)
    for dof in (np.inf,) + tuple(lc.DOFS):
        y = rng.standard_t(1.5, size=(1, 40)) * 100.0
        l = lc.twin_log_density(np.ones((1, 1)), 0.0, dof, y)
        assert np.all(l == 0.0), dof
    for M in (2, 17, 128):
        y = rng.standard_normal((M, 20)) * 3.0
        assert np.all(lc.twin_log_density(np.eye(M), 0.0, np.inf, y) == 0.0)


def test_model_constant_and_factor():
    assert lc.model_constant(1, 3.0) == 0.0 and lc.model_constant(5, np.inf) == 0.0
    corr = lc.correlation(4, 0)
    models = sd._copula_models("t", corr, (3.0, np.inf))
    A, logdet = lc.inverse_factor(corr)
    assert models.A.shape == (2, 4, 4) and np.allclose(models.A[0], A, atol=1e-12) and np.array_equal(models.A[0], models.A[1])
    assert abs(models.logdet[0] - logdet) < 1e-12 and np.array_equal(models.dof, [3.0, np.inf])
    assert np.all(np.triu(models.A[0], 1) == 0.0) and np.allclose(models.corr[0], corr, atol=1e-12)
    # an indefinite matrix is repaired, and the repaired matrix is the one that is inverted
    bad = np.array([[1.0, 0.9, -0.9], [0.9, 1.0, 0.9], [-0.9, 0.9, 1.0]])
    rep = sd._copula_models("t", bad, [np.inf])
    assert np.allclose(rep.A[0] @ rep.corr[0] @ rep.A[0].T, np.eye(3), atol=1e-6)
    one = sd._copula_models("t", [corr, np.eye(4)], (3.0, np.inf))
    assert np.array_equal(one.A[1], np.eye(4)) and one.logdet[1] == 0.0


# ---- host statistics -------------------------------------------------------------------------------------------------------------

def test_likelihood_statistics_against_numpy():
    rng = np.random.default_rng(11)
    L, G = 3, 4
    n = np.array([50, 20, 1])
    d = [rng.standard_normal((G, k)) * (1.0 + l) + 0.3 for l, k in enumerate(n)]
    sums = np.array([x.sum(axis=1) for x in d])
    gram = np.array([x @ x.T for x in d])
    st = sd.likelihood_statistics(n, sums, gram)
    for l in range(2):
        assert np.allclose(st["l_means"][l], d[l].mean(axis=1)) and np.allclose(st["l_vars"][l], d[l].var(axis=1, ddof=1))
        diff = d[l][:, None, :] - d[l][None, :, :]
        assert np.allclose(st["delta_l_means"][l], diff.mean(axis=2))
        assert np.allclose(st["delta_l_vars"][l], diff.var(axis=2, ddof=1), atol=1e-12)
    assert np.all(np.isinf(st["l_vars"][2])) and np.all(np.isinf(st["delta_l_vars"][2]))
    ok = sd.likelihood_statistics(n[:2], sums[:2], gram[:2])
    assert np.allclose(ok["loglik"], sum(d[l].mean(axis=1) for l in range(2)))
    assert np.allclose(ok["var"], sum(d[l].var(axis=1, ddof=1) / n[l] for l in range(2)))
    assert np.allclose(ok["delta"], ok["loglik"][:, None] - ok["loglik"][None, :])
    assert np.allclose(np.diag(ok["delta_var"]), 0.0, atol=1e-14) and np.allclose(ok["delta_var"], ok["delta_var"].T)
    assert ok["delta"].shape == ok["delta_var"].shape == (G, G)
    with pytest.raises(ValueError, match="n \\[L\\], sd \\[L, G\\] and sdd"):
        sd.likelihood_statistics(n, sums, gram[:, 0])


# ---- argument checks, before anything touches the device --------------------------------------------------------------------------

def test_argument_checks():
    u = np.full((2, 5), 0.5)
    for bad in (0.99, 64.5, np.nan, np.inf, None):
        with pytest.raises(ValueError, match="dof must"):
            sd.student_t_quantile(np.zeros(3), bad)
    for dofs in ((0.5, 3), (3, 65), (3, np.nan), ()):
        with pytest.raises(ValueError, match="the grid must hold"):
            sd.copula_log_density(u, np.eye(2), dofs)
    with pytest.raises(ValueError, match="at most 16"):
        sd.copula_log_density(u, np.eye(2), [3.0] * 17)
    with pytest.raises(ValueError, match="u must be \\[M, n\\]"):
        sd.copula_log_density(u[0], np.eye(2), 3)
    with pytest.raises(ValueError, match="one kind and shape"):
        sd.copula_log_density(u, np.eye(2), 3, u_coarse=u[:, :4])
    with pytest.raises(ValueError, match="corr of shape"):
        sd.copula_log_density(u, np.eye(3), 3)
    with pytest.raises(ValueError, match="one correlation matrix"):
        sd.copula_log_density(u, [np.eye(2)] * 3, (3, 4))
    with pytest.raises(ValueError, match="one correlation matrix"):
        sd.copula_log_density(u, np.ones(4), 3)
    with pytest.raises(ValueError, match="unit diagonal"):
        sd.copula_log_density(u, 2.0 * np.eye(2), 3)
    with pytest.raises(ValueError, match="between 1 and 128"):
        sd.copula_log_density(np.full((129, 2), 0.5), np.eye(129), 3)
    with pytest.raises(ValueError, match="no distributions"):
        sd.joint_log_density([], np.zeros((0, 3)), np.eye(1))
    with pytest.raises(ValueError, match="dof must lie in"):
        sd.joint_log_density([object()] * 2, np.zeros((2, 3)), np.eye(2), dof=0.5)
    with pytest.raises(ValueError, match="x must be \\[M, n\\]"):
        sd.joint_log_density([object()] * 2, np.zeros((3, 3)), np.eye(2))
    with pytest.raises(ValueError, match="corr of shape"):
        sd.joint_log_density([object()] * 2, np.zeros((2, 3)), np.eye(3))


class _NoWalk(estimator.Estimate):
    """an Estimate whose quantity must not be touched: the checks under test come first"""

    def __init__(self):
        pass


def test_estimate_argument_checks():
    est = _NoWalk()
    with pytest.raises(ValueError, match="the grid must hold"):
        est.estimate_copula_likelihood(dofs=(0.5, 3), corr=np.eye(2))
    with pytest.raises(ValueError, match="at most 16 grid values"):
        est.estimate_copula_likelihood(dofs=[3.0] * 17, corr=np.eye(2))
    with pytest.raises(ValueError, match="corr must be None, 'scores', 'quadrant'"):
        est.estimate_copula_likelihood(corr="pearson")
    with pytest.raises(ValueError, match="2 correlations for 3 grid values"):
        est.estimate_copula_likelihood(dofs=(3, 4, np.inf), corr=["scores", "quadrant"])
    with pytest.raises(ValueError, match="got an array of shape"):
        est.estimate_copula_likelihood(corr=np.ones(3))
    with pytest.raises(ValueError, match="densities must be the list"):
        est.estimate_copula_likelihood(corr=np.eye(2), densities="scores")


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------

def test_symbols_in_header_version_comment_binding_and_library():
    from mlmc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mlmc_hip.h")).read()
    version_comment = re.search(r"#define MLMC_ABI_VERSION \d+\s*/\*(.*?)\*/", hdr, flags=re.S).group(1)
    lib = _lib.load()
    for name, n_args in ENTRIES.items():
        decl = re.search(r"\bint {}\s*\((.*?)\);".format(name), hdr, flags=re.S)
        assert decl and len(decl.group(1).split(",")) == n_args, name
        assert re.search(r"\b{}\b".format(name), version_comment), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
        assert hasattr(lib, name), name
    assert int(re.search(r"#define MLMC_COPULA_LIK_MAX_M (\d+)", hdr).group(1)) == _lib.COPULA_LIK_MAX_M == 128
    assert int(re.search(r"#define MLMC_COPULA_LIK_MAX_G (\d+)", hdr).group(1)) == _lib.COPULA_LIK_MAX_G == 16


def test_abi_version_stays_8():
    from mlmc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mlmc_hip.h")).read()
    assert int(re.search(r"#define MLMC_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert _lib.ABI_VERSION == 8 and _lib.load().mlmc_abi_version() == 8
