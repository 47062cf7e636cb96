"""GPU tests of the copula pseudo-likelihood through Estimate and tool.simple_distribution: estimate_copula_likelihood on
device-resident storages whose two levels are the Gaussian and the Student-t case of tests/concordance_cases.py (3 degrees of
freedom) under uniform marginals, copula_log_density on device draws of joint_samples, and joint_log_density.

The reference alone clears the bounds: SciPy on the same uniforms at concordance_cases.CORR gives the nearest competitor of the t
case (nu = 4) z = -23.6 and that of the Gaussian case (nu = 30) z = -14.7, against the bound concordance_cases.Z_T_BOUND = 8; the
mean of the Gaussian case is 0.3652 against the closed form -log(det CORR) / 2 = 0.36698."""
import numpy as np
import pytest

from tests import concordance_cases as cc
from tests import score_cases as sk
from tests.test_gpu_concordance_api import _uniform_three
from tests.test_gpu_normal_scores import _densities, _estimate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


@pytest.fixture(scope="module")
def densities():
    return _densities(_uniform_three())


def _report(kind, res):
    print("\n{} case: dof {:g}".format(kind, res.dof))
    for g, ll, se, d, z in zip(res.grid, res.loglik, res.stderr, res.delta, res.z):
        print("  nu {:>4g}: loglik {:.5f} +- {:.5f}, delta {:+.5f}, z {:+.2f}".format(g, ll, se, d, z))


def _checks(res, success, dof, est, densities):
    from mlmc_amd.tool import simple_distribution as sd
    G = len(sd.COPULA_DOF_GRID)
    best = list(res.grid).index(dof)
    others = np.arange(G) != best
    assert res.dof == dof and np.array_equal(res.grid, np.array(sd.COPULA_DOF_GRID, dtype=np.float64))
    assert res.z[best] == 0.0 and res.delta[best] == 0.0 and np.all(res.z[others] < -cc.Z_T_BOUND)
    assert np.all(res.delta[others] < 0.0) and np.all(res.delta_stderr[others] > 0.0)
    assert np.allclose(res.delta, res.loglik - res.loglik[best], rtol=0, atol=1e-12)
    assert res.l_means.shape == res.l_vars.shape == (2, G) and res.corr.shape == (G, 3, 3) and np.all(success)
    assert np.allclose(res.loglik, res.l_means.sum(axis=0)) and np.all(res.stderr > 0.0)
    ref = est.estimate_score_correlation(densities=densities)
    assert np.array_equal(res.n_samples, ref.n_samples) and np.array_equal(res.n_rm_samples, ref.n_rm_samples)


def test_t_case_recovers_three_degrees_of_freedom(hip, densities):
    est = _estimate(cc.copula_levels("t"))
    res, success = est.estimate_copula_likelihood(densities=densities)
    _report("t", res)
    _checks(res, success, float(cc.T_DOF), est, densities)
    # at the copula's own correlation, and a second run repeats bit for bit
    known, _ = est.estimate_copula_likelihood(corr=cc.CORR, densities=densities)
    _report("t, corr known,", known)
    assert known.dof == cc.T_DOF and np.all(known.z[known.grid != cc.T_DOF] < -cc.Z_T_BOUND)
    again, _ = est.estimate_copula_likelihood(corr=cc.CORR, densities=densities)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(known, again))
    # one correlation per grid entry
    per = ["scores" if g == np.inf else "quadrant" for g in res.grid]
    mixed, _ = est.estimate_copula_likelihood(corr=per, densities=densities)
    assert mixed.dof == cc.T_DOF and np.array_equal(mixed.loglik[:-1], res.loglik[:-1])
    assert not np.array_equal(mixed.corr[-1], mixed.corr[0]) and np.array_equal(mixed.corr[0], res.corr[0])
    # a grid of the caller's
    small, _ = est.estimate_copula_likelihood(dofs=(np.inf, 3.0), corr=cc.CORR, densities=densities)
    assert small.dof == 3.0 and small.z[0] < -cc.Z_T_BOUND
    assert np.allclose(small.loglik, known.loglik[[10, 1]], rtol=1e-12)


def test_gaussian_case_recovers_the_gaussian_copula(hip, densities):
    est = _estimate(cc.copula_levels("gauss"))
    res, success = est.estimate_copula_likelihood(densities=densities)
    _report("Gaussian", res)
    _checks(res, success, np.inf, est, densities)
    exact = -0.5 * np.log(np.linalg.det(cc.CORR))
    assert abs(exact - 0.36698) < 1e-5 and abs(res.loglik[-1] - 0.36698) <= 5.0 * res.stderr[-1]
    known, _ = est.estimate_copula_likelihood(corr=cc.CORR, densities=densities)
    _report("Gaussian, corr known,", known)
    assert known.dof == np.inf and np.all(known.z[:-1] < -cc.Z_T_BOUND)
    assert abs(known.loglik[-1] - 0.36698) <= 5.0 * known.stderr[-1]


def test_log_density_of_joint_draws_peaks_at_their_degrees_of_freedom(hip):
    import torch
    from mlmc_amd.tool import simple_distribution as sd
    M, n = 6, 2 ** 14
    corr = np.full((M, M), 0.5)
    np.fill_diagonal(corr, 1.0)
    distrs = [sk.closed_distribution(0.0, (0.0, 1.0)) for _ in range(M)]
    draws = sd.joint_samples(distrs, n, 20261021, corr=corr, dof=3, device=True)
    assert isinstance(draws, torch.Tensor) and draws.is_cuda and tuple(draws.shape) == (M, n)
    ll = sd.copula_log_density(draws, corr, sd.COPULA_DOF_GRID)      # uniform marginals: the draws are their own uniforms
    mean = ll.mean(axis=1)
    print("\nmean log density over the grid:", " ".join("{:g}:{:.4f}".format(g, m) for g, m in zip(sd.COPULA_DOF_GRID, mean)))
    assert ll.shape == (len(sd.COPULA_DOF_GRID), n) and np.all(np.isfinite(ll))
    assert sd.COPULA_DOF_GRID[int(np.argmax(mean))] == 3


def test_joint_log_density_is_the_sum_of_its_parts(hip):
    from mlmc_amd.tool import simple_distribution as sd
    from tests.test_gpu_normal_scores import _closed_three
    distrs = _closed_three()
    rng = np.random.default_rng(4)
    a = np.array([d.domain[0] for d in distrs])
    b = np.array([d.domain[1] for d in distrs])
    x = a[:, None] + (b - a)[:, None] * rng.random((3, 40))
    x[1, 3], x[0, 7], x[2, 9] = np.nan, a[0], b[2] + 1.0
    outside = [3, 7, 9]
    for dof in (None, 4.5):
        got = sd.joint_log_density(distrs, x, cc.CORR, dof=dof)
        ok = np.ones(40, dtype=bool)
        ok[outside] = False
        assert got.shape == (40,) and np.all(np.isnan(got[~ok])) and np.all(np.isfinite(got[ok]))
        u = np.stack(sd.cdfs_on_rule(distrs, list(x[:, ok])))
        rho = np.stack(sd.densities(distrs, list(x[:, ok])))
        want = sd.copula_log_density(u, cc.CORR, np.inf if dof is None else dof)[0] + np.sum(np.log(rho), axis=0)
        assert np.array_equal(got[ok], want)
    # the Gaussian copula at the identity is independence: the sum of the marginal log densities
    indep = sd.joint_log_density(distrs, x[:, ok], np.eye(3))
    assert np.array_equal(indep, np.sum(np.log(rho), axis=0))
