"""GPU tests of mixing="conditioned" in the entries above the C ABI: `joint_probabilities` with the rarest component
not first, Estimate.estimate_joint_exceedance at moderate and at deep thresholds, and the scenarios of `event_samples`, on the storage
of tests/test_gpu_t_copula_api.py (two levels of t-copula samples with 3 degrees of freedom under uniform marginals)."""
import numpy as np
import pytest
from scipy import special, stats

from tests import concordance_cases as cc
from tests import t_lead_cases as tl
from tests.test_gpu_t_copula_api import densities, hip, t_estimate  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DOF = float(cc.T_DOF)
SEEDS = tuple(range(8))
CLOSED_FORM_ABS = 1e-9                                 # the accuracy of bivariate_t_orthant itself (tests/test_gpu_t_box_api.py)


def _sd():
    from mlmc_amd.tool import simple_distribution
    return simple_distribution


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _gate(got, stderr, exact, what, extra=1e-13):
    print("\n{}: {:.10g} +- {:.2g}, exact {:.10g}: off by {:.2f} stderr".format(what, got, stderr, exact, abs(got - exact) / stderr))
    assert abs(got - exact) <= 6.0 * stderr + extra, what


def test_rarest_component_not_first(hip, densities):
    sd = _sd()
    distrs = [d[0] for d in densities]
    q = sd.quantiles(distrs[:2], [np.array([0.99, 0.999])] * 2)
    lower = np.array([[q[0][0], q[1][1], -np.inf]])
    res = sd.joint_probabilities(distrs, lower, np.inf, 2 ** 12, SEEDS, corr=cc.CORR, dof=DOF, mixing="conditioned")
    # the pre-permuted problem: the rarest component first, the unconstrained one left out
    pre = sd.joint_probabilities([distrs[1], distrs[0]], lower[:, [1, 0]], np.inf, 2 ** 12, SEEDS, corr=cc.CORR[np.ix_([1, 0], [1, 0])],
                                 dof=DOF, mixing="conditioned")
    assert _same(res.replicates, pre.replicates) and _same(res.prob, pre.prob)
    # the caller's order as it stands leads with component 0: other bits, the same number
    scores = sd.t_scores(special.ndtri(np.array([0.99, 0.999])), DOF)
    low = sd.correlation_factor(cc.CORR[:2, :2])[0]
    as_given = sd.copula_box_probabilities(low, scores, np.inf, 2 ** 12, SEEDS, dof=DOF, mixing="conditioned")
    assert not _same(as_given.replicates, res.replicates)
    exact = float(sd.bivariate_t_orthant(scores[0], scores[1], cc.CORR[0, 1], DOF))
    _gate(res.prob[0], res.stderr[0], exact, "levels 0.99 and 0.999, the rarer one second", CLOSED_FORM_ABS)
    _gate(as_given.prob[0], as_given.stderr[0], exact, "the same with component 0 leading", CLOSED_FORM_ABS)
    # boxes with different leads in one call: each equals its own call
    both = np.array([[q[0][0], q[1][1], -np.inf], [q[0][1], q[1][0], -np.inf]])
    two = sd.joint_probabilities(distrs, both, np.inf, 2 ** 12, SEEDS, corr=cc.CORR, dof=DOF, mixing="conditioned")
    alone = sd.joint_probabilities(distrs, both[1], np.inf, 2 ** 12, SEEDS, corr=cc.CORR, dof=DOF, mixing="conditioned")
    assert _same(two.replicates[:, 0], res.replicates[:, 0]) and _same(two.replicates[:, 1], alone.replicates[:, 0])


def test_exceedance(t_estimate, densities):
    sd = _sd()
    distrs = [d[0] for d in densities]
    q = sd.quantiles(distrs[:2], [np.array([0.99])] * 2)
    t = np.array([q[0][0], q[1][0], -np.inf])
    res, ok = t_estimate.estimate_joint_exceedance(t, corr=cc.CORR, densities=densities, dof=DOF, mixing="conditioned")
    plain, _ = t_estimate.estimate_joint_exceedance(t, corr=cc.CORR, densities=densities, dof=DOF)
    h = float(stats.t.ppf(0.99, DOF))
    exact = float(sd.bivariate_t_orthant(h, h, cc.CORR[0, 1], DOF))
    assert ok.all() and res.n == 2 ** 14 and res.replicates.shape == (8, 1) and abs(exact - 3.9118e-3) < 1e-7
    _gate(res.prob[0], res.stderr[0], exact, "two 0.99-quantiles, conditioned", CLOSED_FORM_ABS)
    print("plain mixing: {:.10g} +- {:.2g}".format(plain.prob[0], plain.stderr[0]))
    assert res.stderr[0] < plain.stderr[0]
    # two 1 - 1e-6 quantiles of components 0 and 2 (correlation 1 / 2): the M = 2 reference under equicorrelation
    assert cc.CORR[0, 2] == 0.5
    q = sd.quantiles([distrs[0], distrs[2]], [np.array([1.0 - 1e-6])] * 2)
    t = np.array([q[0][0], -np.inf, q[1][0]])
    deep, _ = t_estimate.estimate_joint_exceedance(t, n=2 ** 12, corr=cc.CORR, densities=densities, dof=DOF, mixing="conditioned")
    plain, _ = t_estimate.estimate_joint_exceedance(t, n=2 ** 12, corr=cc.CORR, densities=densities, dof=DOF)
    print("plain mixing at 1e-6: {:.6g} +- {:.2g}".format(plain.prob[0], plain.stderr[0]))
    _gate(deep.prob[0], deep.stderr[0], tl.EQUI[(2, 3.0, 1e-6)], "two 1 - 1e-6 quantiles, conditioned")
    assert deep.stderr[0] / deep.prob[0] <= 1.5 * tl.TWIN[("equi", 2, 3.0, 1e-6)][1]


def test_event_scenarios(t_estimate, densities):
    sd = _sd()
    distrs = [d[0] for d in densities]
    n = 2 ** 12
    q = sd.quantiles(distrs, [np.array([0.5, 0.999])] * 3)
    # box 0: components 0 and 1 above their 0.999-quantiles; box 1: component 2 leads (two-sided), component 0 mild
    lower = np.array([[q[0][1], q[1][1], -np.inf], [q[0][0], -np.inf, q[2][0]]])
    upper = np.array([[np.inf, np.inf, np.inf], [np.inf, np.inf, q[2][1]]])
    scen, ok = t_estimate.sample_given_event(n, lower, upper, corr=cc.CORR, densities=densities, dof=DOF, mixing="conditioned")
    plain, _ = t_estimate.sample_given_event(n, lower, upper, corr=cc.CORR, densities=densities, dof=DOF)
    assert ok.all() and scen.draws.shape == (8, 2, 3, n) and scen.weights.shape == (8, 2, n)
    lo, hi = lower[None, :, :, None], upper[None, :, :, None]
    assert np.all((scen.draws > lo) & (scen.draws < hi))                                    # every scenario lies inside the event
    # rows are in component order: each is the quantile of its own component at its own uniforms
    want = sd.quantiles(distrs, [np.ascontiguousarray(scen.uniforms[:, :, m, :]) for m in range(3)])
    for m in range(3):
        assert _same(scen.draws[:, :, m, :], want[m])
    prob = sd.joint_probabilities(distrs, lower, upper, n, SEEDS, corr=cc.CORR, dof=DOF, mixing="conditioned")
    assert _same(scen.prob.replicates, prob.replicates)                                     # the same leads, the same chain
    # ess / n of the 0.999-quantile event against the twin on the same points (chain order 0, 1, 2; default streams)
    h = float(sd.t_scores(special.ndtri(0.999), DOF))
    L = sd.correlation_factor(cc.CORR)[0]
    t_lo, t_hi = np.array([h, h, -np.inf]), np.full(3, np.inf)
    twin = np.array([tl.lead_twin(L, t_lo, t_hi, DOF, *tl.points_of(s, 3, 0, n, True, draws=True), draws=True)[0] for s in SEEDS])
    ess, ess_twin, ess_plain = scen.ess[:, 0] / n, tl.ess_fraction(twin), plain.ess[:, 0] / n
    print("\ness / n at the 0.999-quantile event: conditioned {:.4f}, twin {:.4f}, plain mixing {:.4f}".format(
        ess.mean(), ess_twin.mean(), ess_plain.mean()))
    assert np.all(ess >= 0.5 * ess_twin)
    means, _ = t_estimate.estimate_event_means(lower, upper, n=n, corr=cc.CORR, densities=densities, dof=DOF, mixing="conditioned")
    assert _same(means.mean, scen.means()[0]) and _same(means.prob.replicates, scen.prob.replicates)
    summary, _ = t_estimate.estimate_aggregates(weights=np.ones(3), n=n, event=(lower, upper), corr=cc.CORR, densities=densities, dof=DOF,
                                                mixing="conditioned")
    assert _same(summary.prob.replicates, scen.prob.replicates)
