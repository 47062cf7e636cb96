"""GPU tests of the Student-t copula through Estimate: estimate_copula_dof, estimate_tail_dependence(dof=...),
estimate_quadrant_correlation, sample_joint(dof=...) and estimate_aggregates(dof=...) on a device-resident storage whose two
levels are the Student-t case of tests/concordance_cases.py (3 degrees of freedom) under uniform marginals."""
import numpy as np
import pytest

from tests import concordance_cases as cc
from tests import t_copula_cases as tc
from tests.test_gpu_concordance_api import _uniform_three
from tests.test_gpu_normal_scores import _densities, _estimate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


@pytest.fixture(scope="module")
def t_estimate(hip):
    return _estimate(cc.copula_levels("t"))


@pytest.fixture(scope="module")
def densities():
    return _densities(_uniform_three())


def test_copula_dof_is_found(t_estimate, densities):
    fit, res = t_estimate.estimate_copula_dof(corr=cc.CORR, densities=densities)
    print("\nobjective over the grid:", " ".join("{:g}:{:.1f}".format(g, o) for g, o in zip(fit.grid, fit.objective)))
    assert fit.dof == cc.T_DOF
    assert fit.z.shape == (len(fit.grid), 4, 3, 3) and res.z.shape == (4, 3, 3)                 # tail="both": two events per level
    assert np.array_equal(res.z, fit.z[list(fit.grid).index(3.0)], equal_nan=True)
    upper, _ = t_estimate.estimate_copula_dof(tail="upper", corr=cc.CORR, densities=densities)
    assert upper.dof == cc.T_DOF and upper.z.shape[1] == 2
    with_quadrant, _ = t_estimate.estimate_copula_dof(corr="quadrant", densities=densities)
    assert with_quadrant.dof == cc.T_DOF


def test_tail_dependence_under_the_t_model(t_estimate, densities):
    gauss = t_estimate.estimate_tail_dependence(probs=cc.PROBS, corr=cc.CORR, densities=densities)
    t = t_estimate.estimate_tail_dependence(probs=cc.PROBS, corr=cc.CORR, densities=densities, dof=cc.T_DOF)
    z_g, z_t = cc.off_diagonal(gauss.z), cc.off_diagonal(t.z)
    print(f"\nz under the Gaussian model {np.array2string(z_g, precision=3)}, under the t model {np.array2string(z_t, precision=3)}")
    assert np.all(z_g[0] > cc.Z_T_BOUND) and np.all(np.abs(z_t) < cc.Z_BOUND)
    # the counts do not depend on the model, and dof=None / inf is the call as it has always been
    assert np.array_equal(t.prob, gauss.prob) and np.array_equal(t.var, gauss.var)
    inf = t_estimate.estimate_tail_dependence(probs=cc.PROBS, corr=cc.CORR, densities=densities, dof=np.inf)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(inf[:7], gauss[:7]))
    assert np.array_equal(gauss.model, cc.model_orthant(cc.PROBS, cc.CORR))


def test_quadrant_correlation(t_estimate, densities):
    res = t_estimate.estimate_quadrant_correlation(densities=densities)
    iu = np.triu_indices(3, 1)
    print("\nquadrant correlation", res.corr[iu], "stderr", res.stderr[iu])
    assert np.all(np.abs(res.corr[iu] - cc.CORR[iu]) <= 5.0 * res.stderr[iu]) and np.all(res.stderr[iu] < 0.01)
    assert np.all(np.diag(res.corr) == 1.0) and np.array_equal(res.corr, res.corr.T)
    assert res.prob.shape == res.var.shape == (3, 3) and res.counts.pair.shape == (2, 1, 3, 3, 3)
    assert np.allclose(np.diag(res.prob), 0.5, atol=0.01)


def test_sample_joint_with_the_quadrant_correlation(t_estimate, densities):
    from mlmc_amd.tool import simple_distribution as sd
    n = tc.STAT_N
    draws, success, used = t_estimate.sample_joint(n, tc.STAT_SEED, corr="quadrant", densities=densities, dof=cc.T_DOF, device=True)
    assert tuple(draws.shape) == (3, n) and np.all(success) and np.max(np.abs(used - cc.CORR)) < 0.03
    # uniform marginals: the draws are their own uniforms
    lower, upper = cc.upper_events(tc.STAT_PROBS, 3)
    counts = sd.concordance_counts(draws, None, lower, upper)
    # the draws follow the correlation that was used, the repaired estimate: the models are evaluated there
    res = tc.concordance_z(counts.pair, counts.kept[0], corr=used)
    print("\n|z| under the t model", np.round(np.abs(res["z_t"]).max(axis=1), 2), "z under the Gaussian model at 0.9",
          np.round(res["z_gauss"][1], 2))
    assert np.max(np.abs(res["z_t"])) < tc.STAT_Z_BOUND and np.min(res["z_gauss"][1]) > tc.STAT_Z_GAUSS


def test_aggregates_equal_the_aggregates_of_the_draws(t_estimate, densities):
    from mlmc_amd.tool import simple_distribution as sd
    distrs = [d[0] for d in densities]
    kw = dict(weights=np.ones(3), probs=(0.05, 0.5, 0.95), n=512, seeds=(3, 4), corr=cc.CORR, densities=densities, qmc=False)
    a, _ = t_estimate.estimate_aggregates(block=2 ** 20, dof=3, **kw)
    b, _ = t_estimate.estimate_aggregates(block=100, dof=3, **kw)
    for name, x, y in zip(a._fields, a, b):
        if x is None or name in ("names", "prob"):
            assert (x is None and y is None) or list(x) == list(y), name
        else:
            assert np.array_equal(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), equal_nan=True), name
    for block in (2 ** 20, 100):
        rows = sd.joint_aggregates(distrs, 512, 3, weights=np.ones(3), extremes=("max", "min", "argmax", "argmin"), corr=cc.CORR, dof=3,
                                   block=block).rows
        want = sd.scenario_aggregates(sd.joint_samples(distrs, 512, 3, corr=cc.CORR, dof=3), weights=np.ones(3),
                                      extremes=("max", "min", "argmax", "argmin")).rows
        assert np.array_equal(rows, want)
    gauss, _ = t_estimate.estimate_aggregates(block=2 ** 20, **kw)
    assert not np.array_equal(np.asarray(gauss.quantiles), np.asarray(a.quantiles))
    with pytest.raises(ValueError, match="dof together with given"):
        t_estimate.estimate_aggregates(dof=3, given={0: 0.5}, **kw)
