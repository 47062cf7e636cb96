"""GPU tests of the Student-t copula in the joint numbers of Estimate: estimate_joint_probability / _exceedance(dof=...),
sample_given_event / estimate_event_means(dof=...), estimate_aggregates(dof=..., event=...) and the bootstrap band, on the storage of
tests/test_gpu_t_copula_api.py (two levels of t-copula samples with 3 degrees of freedom under uniform marginals).  The boxes are
chosen on the CPU from the closed forms bivariate_t_orthant / bivariate_orthant."""
import numpy as np
import pytest
from scipy import special, stats

from tests import concordance_cases as cc
from tests.test_gpu_t_copula_api import densities, hip, t_estimate  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DOF = cc.T_DOF
COUNT_N = 2 ** 16
SEEDS = tuple(range(8))


def _sd():
    from mlmc_amd.tool import simple_distribution
    return simple_distribution


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _cdf2(p, q, rho, dof):
    """P(U_a < p, U_b < q) under the copula, from the orthant of the mirrored scores"""
    sd = _sd()
    if dof is None:
        return float(sd.bivariate_orthant(-special.ndtri(p), -special.ndtri(q), rho))
    return float(sd.bivariate_t_orthant(-stats.t.ppf(p, dof), -stats.t.ppf(q, dof), rho, dof))


def _square(a, rho, dof):
    """P(a < U_1 < 1 - a, a < U_2 < 1 - a)"""
    b = 1.0 - a
    return _cdf2(b, b, rho, dof) - 2.0 * _cdf2(a, b, rho, dof) + _cdf2(a, a, rho, dof)


def _central_box():
    """the central square of components 1 and 2 whose probability under the t copula is nearest to 0.2: there the t copula holds
    more mass than the Gaussian one (both components near their medians at once) -> (a, t value, Gaussian value)"""
    rho = cc.CORR[1, 2]
    grid = np.arange(0.25, 0.36, 0.01)
    t = np.array([_square(a, rho, DOF) for a in grid])
    k = int(np.argmin(np.abs(t - 0.2)))
    return float(grid[k]), float(t[k]), _square(float(grid[k]), rho, None)


def _distrs(densities):
    return [d[0] for d in densities]


def test_agreement_with_counting(t_estimate, densities):
    sd = _sd()
    a, p_t, p_g = _central_box()
    err = np.sqrt(p_t * (1.0 - p_t) / COUNT_N)
    assert 0.15 < p_t < 0.25 and p_t - p_g >= 10.0 * err                                    # chosen on the CPU
    distrs = _distrs(densities)
    lim = sd.quantiles(distrs[1:], [np.array([a, 1.0 - a])] * 2)
    lower, upper = np.array([-np.inf, lim[0][0], lim[1][0]]), np.array([np.inf, lim[0][1], lim[1][1]])
    res, ok = t_estimate.estimate_joint_probability(lower, upper, n=2 ** 12, corr=cc.CORR, densities=densities, dof=DOF)
    gauss, _ = t_estimate.estimate_joint_probability(lower, upper, n=2 ** 12, corr=cc.CORR, densities=densities)
    x, _, _ = t_estimate.sample_joint(COUNT_N, 1234, corr=cc.CORR, densities=densities, dof=DOF)
    frac = np.mean(np.all((x > lower[:, None]) & (x < upper[:, None]), axis=0))
    print("\nsquare ({:g}, {:g})^2: t {:.6f} +- {:.2g} (closed form {:.6f}), counted {:.6f}, Gaussian {:.6f} (closed form {:.6f}), "
          "binomial error {:.2g}".format(a, 1 - a, res.prob[0], res.stderr[0], p_t, frac, gauss.prob[0], p_g, err))
    assert ok.all() and res.prob.shape == (1,) and res.replicates.shape == (8, 1)
    assert abs(frac - res.prob[0]) <= 5.0 * err
    assert abs(gauss.prob[0] - res.prob[0]) > 5.0 * err and abs(frac - gauss.prob[0]) > 5.0 * err
    assert abs(res.prob[0] - p_t) <= 6.0 * res.stderr[0] + 1e-9                               # 1e-9: the closed form's own accuracy
    # the unconstrained component drops: the two-component problem gives the same bits
    sub = sd.joint_probabilities(distrs[1:], lower[1:], upper[1:], 2 ** 12, SEEDS, corr=cc.CORR[1:, 1:], dof=DOF)
    assert _same(sub.replicates, res.replicates)


def test_exceedance(t_estimate, densities):
    sd = _sd()
    distrs = _distrs(densities)
    q = sd.quantiles(distrs[:2], [np.array([0.99])] * 2)
    t = np.array([q[0][0], q[1][0], -np.inf])
    res, _ = t_estimate.estimate_joint_exceedance(t, corr=cc.CORR, densities=densities, dof=DOF)
    gauss, _ = t_estimate.estimate_joint_exceedance(t, corr=cc.CORR, densities=densities)
    h_t, h_g = float(stats.t.ppf(0.99, DOF)), float(special.ndtri(0.99))
    exact_t = float(sd.bivariate_t_orthant(h_t, h_t, cc.CORR[0, 1], DOF))
    exact_g = float(sd.bivariate_orthant(h_g, h_g, cc.CORR[0, 1]))
    ratio, want = res.prob[0] / gauss.prob[0], exact_t / exact_g
    print("\nexceedance of two 0.99-quantiles: t {:.8g} +- {:.2g} (closed form {:.8g}), Gaussian {:.8g} (closed form {:.8g}), "
          "factor {:.4f} (closed forms {:.4f})".format(res.prob[0], res.stderr[0], exact_t, gauss.prob[0], exact_g, ratio, want))
    assert res.n == 2 ** 14 and res.replicates.shape == (8, 1)
    assert abs(res.prob[0] - exact_t) <= 6.0 * res.stderr[0]
    assert want > 2.0 and abs(ratio - want) <= 6.0 * (res.stderr[0] + ratio * gauss.stderr[0]) / gauss.prob[0]
    # lower = thresholds, upper = +inf
    same, _ = t_estimate.estimate_joint_probability(t, np.inf, corr=cc.CORR, densities=densities, dof=DOF)
    assert _same(same.replicates, res.replicates)


def test_event_scenarios(t_estimate, densities):
    sd = _sd()
    distrs = _distrs(densities)
    q = sd.quantiles(distrs[:2], [np.array([0.4, 0.93])] * 2)
    lower = np.array([[q[0][1], q[1][1], -np.inf], [q[0][0], -np.inf, -np.inf]])
    upper = np.array([[np.inf, np.inf, np.inf], [q[0][1], np.inf, np.inf]])
    n = 2 ** 12
    scen, ok = t_estimate.sample_given_event(n, lower, upper, corr=cc.CORR, densities=densities, dof=DOF)
    assert ok.all() and scen.draws.shape == (8, 2, 3, n) and scen.weights.shape == (8, 2, n)
    lo, hi = lower[None, :, :, None], upper[None, :, :, None]
    assert np.all((scen.draws > lo) & (scen.draws < hi))                                    # every draw lies in its event
    want = sd.quantiles(distrs, [np.ascontiguousarray(scen.uniforms[:, :, m, :]) for m in range(3)])
    for m in range(3):
        assert _same(scen.draws[:, :, m, :], want[m])
    prob, _ = t_estimate.estimate_joint_probability(lower, upper, n=n, corr=cc.CORR, densities=densities, dof=DOF)
    assert _same(scen.prob.replicates, prob.replicates)                                     # default streams: the same chain
    # under the t copula even one constrained component has weights that vary: its width depends on the point's mixing scale
    assert np.all(scen.weights > 0) and np.ptp(scen.weights[0, 1]) > 0
    # E[X_2 | X_0, X_1 above their 0.93-quantiles] against the filtered scenarios of sample_joint (a probability of about 0.03)
    means, _ = t_estimate.estimate_event_means(lower[0], upper[0], n=n, corr=cc.CORR, densities=densities, dof=DOF)
    x, _, _ = t_estimate.sample_joint(COUNT_N, 99, corr=cc.CORR, densities=densities, dof=DOF)
    kept = x[:, np.all((x > lower[0][:, None]) & (x < upper[0][:, None]), axis=0)]
    err = np.std(kept[2], ddof=1) / np.sqrt(kept.shape[1])
    gauss, _ = t_estimate.estimate_event_means(lower[0], upper[0], n=n, corr=cc.CORR, densities=densities)
    print("\nevent of probability {:.4f}: {} of {} scenarios kept; E[X_2 | event] {:.5f} +- {:.2g}, filtered {:.5f} +- {:.2g}, "
          "Gaussian copula {:.5f}".format(means.prob.prob[0], kept.shape[1], COUNT_N, means.mean[0, 2], means.stderr[0, 2],
                                          kept[2].mean(), err, gauss.mean[0, 2]))
    assert 0.02 < means.prob.prob[0] < 0.05 and means.mean.shape == (1, 3)
    assert abs(means.mean[0, 2] - kept[2].mean()) <= 5.0 * err
    assert _same(means.mean[0], scen.means()[0][0]) and _same(means.prob.replicates[:, 0], scen.prob.replicates[:, 0])


def test_gaussian_path_unchanged(t_estimate, densities):
    """dof=None and dof=np.inf are the calls as they have always been, bit for bit, on every changed method"""
    sd = _sd()
    distrs = _distrs(densities)
    lower, upper = np.array([0.3, -np.inf, 0.2]), np.array([np.inf, 0.8, 0.9])
    kw = dict(corr=cc.CORR, densities=densities)
    small = dict(n=256, seeds=(0, 1))
    for dof in (None, np.inf):
        a, _ = t_estimate.estimate_joint_probability(lower, upper, dof=dof, **small, **kw)
        b, _ = t_estimate.estimate_joint_probability(lower, upper, **small, **kw)
        assert _same(a.replicates, b.replicates)
        assert _same(a.replicates, sd.joint_probabilities(distrs, lower, upper, 256, (0, 1), corr=cc.CORR).replicates)
        a, _ = t_estimate.estimate_joint_exceedance(lower, dof=dof, **small, **kw)
        b, _ = t_estimate.estimate_joint_exceedance(lower, **small, **kw)
        assert _same(a.replicates, b.replicates)
        a, _ = t_estimate.sample_given_event(256, lower, upper, seeds=(0, 1), dof=dof, **kw)
        b, _ = t_estimate.sample_given_event(256, lower, upper, seeds=(0, 1), **kw)
        ev = sd.event_samples(distrs, lower, upper, 256, (0, 1), corr=cc.CORR)
        for x, y, z in ((a.draws, b.draws, ev.draws), (a.weights, b.weights, ev.weights), (a.uniforms, b.uniforms, ev.uniforms)):
            assert _same(x, y) and _same(x, z)
        a, _ = t_estimate.estimate_event_means(lower, upper, dof=dof, **small, **kw)
        b, _ = t_estimate.estimate_event_means(lower, upper, **small, **kw)
        assert _same(a.mean, b.mean)
        a, _ = t_estimate.estimate_aggregates(weights=np.ones(3), n=256, seeds=(0, 1), event=(lower, upper), dof=dof, **kw)
        b, _ = t_estimate.estimate_aggregates(weights=np.ones(3), n=256, seeds=(0, 1), event=(lower, upper), **kw)
        assert _same(a.quantiles, b.quantiles) and _same(a.prob.replicates, b.prob.replicates)
        boot = dict(n_subsamples=4, seed=5, n=128, seeds=(0, 1), densities=densities)
        a = t_estimate.bootstrap_joint_probability(lower, upper, dof=dof, **boot)
        b = t_estimate.bootstrap_joint_probability(lower, upper, **boot)
        assert _same(a.prob, b.prob) and np.array_equal(a.replicates, b.replicates, equal_nan=True)
        a = t_estimate.bootstrap_joint_exceedance(lower, dof=dof, **boot)
        b = t_estimate.bootstrap_joint_exceedance(lower, **boot)
        assert _same(a.prob, b.prob) and np.array_equal(a.replicates, b.replicates, equal_nan=True)
    # the score entries: the Gaussian call and its default streams
    L = np.linalg.cholesky(cc.CORR)
    a = sd.copula_box_probabilities(L, [-1.0, -0.5, -np.inf], [0.5, np.inf, 1.0], 256, (0, 1), dof=np.inf)
    b = sd.copula_box_probabilities(L, [-1.0, -0.5, -np.inf], [0.5, np.inf, 1.0], 256, (0, 1), streams=[0, 1])
    assert _same(a.replicates, b.replicates)
    a = sd.copula_box_draws(L, [-1.0, -0.5, -np.inf], [0.5, np.inf, 1.0], 256, (0, 1), dof=np.inf)
    b = sd.copula_box_draws(L, [-1.0, -0.5, -np.inf], [0.5, np.inf, 1.0], 256, (0, 1), streams=[0, 1, 2])
    assert _same(a.z, b.z) and _same(a.u, b.u) and _same(a.weights, b.weights)


def test_aggregates_of_an_event_and_the_bootstrap_band(t_estimate, densities):
    lower, upper = np.array([0.8, 0.8, -np.inf]), np.array([np.inf, np.inf, np.inf])
    kw = dict(corr=cc.CORR, densities=densities)
    agg, ok = t_estimate.estimate_aggregates(weights=np.ones(3), n=1024, seeds=(0, 1, 2, 3), event=(lower, upper), dof=DOF, **kw)
    prob, _ = t_estimate.estimate_joint_probability(lower, upper, n=1024, seeds=(0, 1, 2, 3), dof=DOF, **kw)
    gauss, _ = t_estimate.estimate_aggregates(weights=np.ones(3), n=1024, seeds=(0, 1, 2, 3), event=(lower, upper), **kw)
    assert ok.all() and _same(agg.prob.replicates, prob.replicates) and _same(agg.prob.prob, prob.prob)
    assert np.all(np.isfinite(np.asarray(agg.quantiles, dtype=np.float64)))
    assert not _same(np.asarray(agg.quantiles, dtype=np.float64), np.asarray(gauss.quantiles, dtype=np.float64))
    # the band of the exceedance: nu is held fixed over the replicates
    band = t_estimate.bootstrap_joint_exceedance(lower, n_subsamples=8, seed=5, n=256, seeds=(0, 1), densities=densities, dof=DOF)
    base, _ = t_estimate.estimate_joint_exceedance(lower, n=256, seeds=(0, 1), densities=densities, dof=DOF)
    plain = t_estimate.bootstrap_joint_exceedance(lower, n_subsamples=8, seed=5, n=256, seeds=(0, 1), densities=densities)
    print("\nexceedance {:.5f}, band [{:.5f}, {:.5f}] over {} replicates; under the Gaussian copula {:.5f}".format(
        band.prob[0], band.lo[0], band.hi[0], band.n_ok, plain.prob[0]))
    assert _same(band.prob, base.prob) and band.replicates.shape == (8, 1) and band.n_ok == 8
    assert band.lo[0] <= band.prob[0] <= band.hi[0] and band.lo[0] < band.hi[0]
    assert band.prob[0] > plain.prob[0]
