"""GPU tests of the conditional family under the Student-t copula in the components' own units: conditional_probabilities,
conditional_event_samples, conditional_aggregates (tool.simple_distribution) and the Estimate methods above them, on uniform
marginals (Fhat(x) = x up to the rounding of the quadrature, so a t score y is the value T_nu(y)).  The closed-form cases are
those of tests/conditional_t_box_cases.LAWS, which tests/test_conditional_t_box_cpu.py holds within 3 standard errors on the twin."""
import numpy as np
import pytest
from scipy import stats

from tests import box_prob_cases as bc
from tests import concordance_cases as cc
from tests import conditional_t_box_cases as ctc
from tests.test_gpu_concordance_api import _uniform_three
from tests.test_gpu_t_copula_api import densities, hip, t_estimate  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DOF = 3.0
N = 2 ** 12
COUNT_N = 2 ** 16


def _sd():
    from mlmc_amd.tool import simple_distribution
    return simple_distribution


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _units(y, dof=DOF):
    """the value of a uniform marginal whose t score is y; infinite limits stay infinite"""
    y = np.asarray(y, dtype=np.float64)
    return np.where(np.isfinite(y), stats.t.cdf(y, dof), y)


@pytest.fixture(scope="module")
def uniform(hip):
    return _uniform_three()


@pytest.mark.parametrize("law", ctc.LAWS, ids=repr)
def test_closed_forms(uniform, law):
    """(i) q = 1 against the difference of conditional_cdfs at the two limits, (ii) q = 2 given p = 1 against dblquad, (iii) C = I
    with an extreme given value; each within 5 standard errors of the call's 8 seeds at n = 2^12"""
    sd = _sd()
    M = law.corr.shape[0]
    distrs = uniform[:M]
    given = {0: float(_units(law.y0, law.dof))}
    lower, upper = _units(law.lo, law.dof), _units(law.hi, law.dof)
    res = sd.conditional_probabilities(distrs, lower, upper, given, N, bc.SEEDS8, corr=law.corr, dof=law.dof)
    exact = law.reference()
    if law.name == "one":
        cdf = sd.conditional_cdfs(distrs, np.array([lower[0], upper[0]]), given, law.corr, dof=law.dof)
        # the two closed forms agree: the limits carry the 3e-11 relative error of t_scores and the rounding of the quadrature
        assert abs((cdf[0, 1] - cdf[0, 0]) - exact) < 1e-8
        exact = float(cdf[0, 1] - cdf[0, 0])
    off = abs(res.prob[0] - exact) / res.stderr[0]
    print("\n{}: {:.10f} +- {:.2g}, reference {:.10f}, off by {:.2f} standard errors".format(law.name, res.prob[0], res.stderr[0], exact, off))
    assert res.prob.shape == (1,) and res.replicates.shape == (8, 1) and res.n == N
    assert abs(res.prob[0] - exact) <= 5.0 * res.stderr[0]
    if law.name == "eye":
        # the Gaussian copula cannot widen: its conditional probability is the unconditional one
        gauss = sd.conditional_probabilities(distrs, lower, upper, given, N, bc.SEEDS8, corr=law.corr)
        plain = sd.joint_probabilities(distrs, np.concatenate([[-np.inf], lower]), np.concatenate([[np.inf], upper]), N, bc.SEEDS8,
                                       corr=law.corr)
        print("Gaussian copula: conditional {:.10f}, unconditional {:.10f}".format(gauss.prob[0], plain.prob[0]))
        assert abs(gauss.prob[0] - plain.prob[0]) <= 1e-12 and abs(gauss.prob[0] - (upper[0] - lower[0])) < 1e-8
        assert abs(gauss.prob[0] - res.prob[0]) > 0.1


def _two(uniform):
    law = ctc.LAWS[1]
    given = {0: float(_units(law.y0))}
    return law, uniform, given, _units(law.lo), _units(law.hi)


def test_agreement_with_counting(uniform):
    sd = _sd()
    law, distrs, given, lower, upper = _two(uniform)
    res = sd.conditional_probabilities(distrs, lower, upper, given, N, bc.SEEDS8, corr=law.corr, dof=DOF)
    x = sd.conditional_samples(distrs, COUNT_N, 1234, given, corr=law.corr, dof=DOF)
    assert x.shape == (3, COUNT_N) and np.all(x[0] == given[0])
    frac = float(np.mean(np.all((x[1:] > lower[:, None]) & (x[1:] < upper[:, None]), axis=0)))
    err = np.sqrt(frac * (1.0 - frac) / COUNT_N)
    gauss = sd.conditional_probabilities(distrs, lower, upper, given, N, bc.SEEDS8, corr=law.corr)
    print("\nconditional box: t {:.6f} +- {:.2g}, counted {:.6f} +- {:.2g}, Gaussian copula {:.6f}".format(
        res.prob[0], res.stderr[0], frac, err, gauss.prob[0]))
    assert abs(res.prob[0] - frac) <= 5.0 * err


def test_event_scenarios(uniform):
    sd = _sd()
    law, distrs, given, lower, upper = _two(uniform)
    lo3, hi3 = np.concatenate([[-np.inf], lower]), np.concatenate([[np.inf], upper])
    scen = sd.conditional_event_samples(distrs, lo3, hi3, given, N, bc.SEEDS8, corr=law.corr, dof=DOF)
    assert scen.draws.shape == (8, 1, 3, N) and scen.weights.shape == (8, 1, N) and scen.ok.all()
    assert np.all((scen.draws[:, :, 1:] > lower[None, None, :, None]) & (scen.draws[:, :, 1:] < upper[None, None, :, None]))
    assert np.all(scen.draws[:, :, 0, :] == given[0])                                       # rows of given components
    want = sd.quantiles(distrs, [np.ascontiguousarray(scen.uniforms[:, :, m, :]) for m in range(3)])
    for m in (1, 2):
        assert _same(scen.draws[:, :, m, :], want[m])
    u0 = sd.normal_scores(distrs[:1], np.array([[given[0]]]), return_uniforms=True)[1][0, 0]
    assert np.all(scen.uniforms[:, :, 0, :] == u0)
    # both free components are constrained, so no component is dropped: the same chain under default streams
    prob = sd.conditional_probabilities(distrs, lower, upper, given, N, bc.SEEDS8, corr=law.corr, dof=DOF)
    assert _same(scen.prob.replicates, prob.replicates)
    assert np.all(scen.weights > 0) and np.ptp(scen.weights[0, 0]) > 0
    # E[X_m | event, given]: means() within 5 of ITS OWN standard errors.  The mean of the conditional_samples draws that fall
    # inside the event has a standard error some hundred times that of means(), so means() is held against the value that mean
    # estimates, the quadrature ctc.EVENT_MEANS_B (good to 1e-9), and the mean of the kept draws is held against the same value
    # within 5 of its standard errors: the two estimate one number, and means() meets the bound on it
    mean, stderr = scen.means()
    x = sd.conditional_samples(distrs, COUNT_N, 99, given, corr=law.corr, dof=DOF)
    kept = x[:, np.all((x[1:] > lower[:, None]) & (x[1:] < upper[:, None]), axis=0)]
    assert kept.shape[1] > 1000
    for m in (1, 2):
        exact = ctc.EVENT_MEANS_B[m - 1]
        err = np.std(kept[m], ddof=1) / np.sqrt(kept.shape[1])
        print("\nE[X_{} | event, given] {:.9f} +- {:.2g} ({:.2f} standard errors from the quadrature {:.9f}), from {} kept draws "
              "{:.6f} +- {:.2g}".format(m, mean[0, m], stderr[0, m], abs(mean[0, m] - exact) / stderr[0, m], exact, kept.shape[1],
                                        kept[m].mean(), err))
        assert abs(mean[0, m] - exact) <= 5.0 * stderr[0, m]
        assert abs(kept[m].mean() - exact) <= 5.0 * err
    assert abs(mean[0, 0] - given[0]) < 1e-12


def test_aggregates_equal_the_aggregates_of_the_draws(uniform):
    sd = _sd()
    law, distrs, _, _, _ = _two(uniform)
    n = 1000
    given = {0: np.array([0.9, 0.999])}
    kw = dict(weights=np.ones(3), lower=[-np.inf, 0.2, 0.2], upper=[np.inf, 0.9, 0.9], extremes=("max", "argmin"))
    draws = sd.conditional_samples(distrs, n, 7, given, corr=law.corr, dof=DOF)
    want = sd.scenario_aggregates(draws, **kw)
    assert draws.shape == (2, 3, n)
    for block in (2 ** 20, 100):
        got = sd.conditional_aggregates(distrs, n, 7, given, corr=law.corr, dof=DOF, block=block, **kw)
        assert got.names == want.names and got.rows.shape == (2, len(want.names), n) and _same(got.rows, want.rows)
    # without dof: joint_aggregates(given=...), the same body
    a = sd.conditional_aggregates(distrs, n, 7, given, corr=law.corr, block=100, **kw)
    b = sd.joint_aggregates(distrs, n, 7, given=given, corr=law.corr, block=100, **kw)
    assert _same(a.rows, b.rows) and not _same(a.rows, want.rows)


def test_dof_none_is_the_call_with_given(uniform):
    sd = _sd()
    law, distrs, given, lower, upper = _two(uniform)
    lo3, hi3 = np.concatenate([[-np.inf], lower]), np.concatenate([[np.inf], upper])
    for dof in (None, np.inf):
        a = sd.conditional_probabilities(distrs, lower, upper, given, 256, (0, 1), corr=law.corr, dof=dof)
        b = sd.joint_probabilities(distrs, lower, upper, 256, (0, 1), corr=law.corr, given=given)
        assert _same(a.replicates, b.replicates)
        a = sd.conditional_event_samples(distrs, lo3, hi3, given, 256, (0, 1), corr=law.corr, dof=dof)
        b = sd.event_samples(distrs, lo3, hi3, 256, (0, 1), corr=law.corr, given=given)
        assert _same(a.draws, b.draws) and _same(a.weights, b.weights) and _same(a.uniforms, b.uniforms)


def test_estimate(t_estimate, densities):
    """every new method: with dof None the existing method with given=, bit for bit; with dof the simple_distribution call on the
    same densities and correlation"""
    sd = _sd()
    est = t_estimate
    distrs = [d[0] for d in densities]
    given = {0: 0.97}
    lower, upper = np.array([0.6, -np.inf]), np.array([np.inf, 0.8])
    lo3, hi3 = np.concatenate([[-np.inf], lower]), np.concatenate([[np.inf], upper])
    kw = dict(corr=cc.CORR, densities=densities)
    small = dict(n=256, seeds=(0, 1))
    a, ok = est.estimate_conditional_probability(lower, upper, given, **small, **kw)
    b, _ = est.estimate_joint_probability(lower, upper, given=given, **small, **kw)
    assert ok.all() and _same(a.replicates, b.replicates)
    t, _ = est.estimate_conditional_probability(lower, upper, given, dof=DOF, **small, **kw)
    assert _same(t.replicates, sd.conditional_probabilities(distrs, lower, upper, given, 256, (0, 1), corr=cc.CORR, dof=DOF).replicates)
    assert not _same(t.replicates, a.replicates)
    a, _ = est.estimate_conditional_exceedance(lower, given, **small, **kw)
    b, _ = est.estimate_joint_exceedance(lower, given=given, **small, **kw)
    assert _same(a.replicates, b.replicates)
    t, _ = est.estimate_conditional_exceedance(lower, given, dof=DOF, **small, **kw)
    assert _same(t.replicates, sd.conditional_probabilities(distrs, lower, np.inf, given, 256, (0, 1), corr=cc.CORR, dof=DOF).replicates)
    a, _ = est.sample_conditional_event(256, lo3, hi3, given, seeds=(0, 1), **kw)
    b, _ = est.sample_given_event(256, lo3, hi3, given=given, seeds=(0, 1), **kw)
    assert _same(a.draws, b.draws) and _same(a.weights, b.weights) and _same(a.uniforms, b.uniforms)
    t, _ = est.sample_conditional_event(256, lo3, hi3, given, seeds=(0, 1), dof=DOF, **kw)
    ev = sd.conditional_event_samples(distrs, lo3, hi3, given, 256, (0, 1), corr=cc.CORR, dof=DOF)
    assert _same(t.draws, ev.draws) and _same(t.weights, ev.weights) and _same(t.prob.replicates, ev.prob.replicates)
    a, _ = est.estimate_conditional_event_means(lo3, hi3, given, **small, **kw)
    b, _ = est.estimate_event_means(lo3, hi3, given=given, **small, **kw)
    assert _same(a.mean, b.mean) and _same(a.stderr, b.stderr)
    t, _ = est.estimate_conditional_event_means(lo3, hi3, given, dof=DOF, **small, **kw)
    assert _same(t.mean, ev.means()[0]) and _same(t.prob.replicates, ev.prob.replicates)
    agg = dict(weights=np.ones(3), n=256, seeds=(0, 1))
    a, _ = est.estimate_conditional_aggregates(given, **agg, **kw)
    b, _ = est.estimate_aggregates(given=given, **agg, **kw)
    assert _same(a.quantiles, b.quantiles) and _same(a.mean, b.mean)
    a, _ = est.estimate_conditional_aggregates(given, event=(lo3, hi3), **agg, **kw)
    b, _ = est.estimate_aggregates(given=given, event=(lo3, hi3), **agg, **kw)
    assert _same(a.quantiles, b.quantiles) and _same(a.prob.replicates, b.prob.replicates)
    # with dof: every row (the linear one, the extremes and their indices) against conditional_aggregates of the same seeds; the
    # quantiles are np.percentile of a row bit for bit, the means are sums in another order
    t, _ = est.estimate_conditional_aggregates(given, dof=DOF, **agg, **kw)
    rows = [sd.conditional_aggregates(distrs, 256, seed, given, corr=cc.CORR, dof=DOF, qmc=True, weights=np.ones(3),
                                      extremes=("max", "min", "argmax", "argmin")).rows for seed in (0, 1)]
    assert tuple(t.names) == ("linear0", "max", "min", "argmax", "argmin") and rows[0].shape == (5, 256)
    want_q = np.stack([np.percentile(r, 100.0 * t.probs, axis=1).T for r in rows]).mean(axis=0)
    assert t.quantiles.shape == (5, 3) and np.array_equal(t.quantiles, want_q)
    assert np.allclose(t.mean, np.stack([r.mean(axis=1) for r in rows]).mean(axis=0), rtol=0, atol=1e-12)
    assert np.allclose(t.worst_prob, np.stack([[np.mean(r[3] == m) for m in range(3)] for r in rows]).mean(axis=0), rtol=0, atol=1e-12)
    g, _ = est.estimate_conditional_aggregates(given, **agg, **kw)
    assert not np.array_equal(t.quantiles, g.quantiles)
    # with dof and an event: the scenarios of conditional_event_samples, their probability and the mean of the total
    t, _ = est.estimate_conditional_aggregates(given, event=(lo3, hi3), dof=DOF, **agg, **kw)
    assert _same(t.prob.replicates, ev.prob.replicates)
    assert abs(t.mean[0, 0] - ev.means()[0][0].sum()) < 1e-10
    # corr="quadrant", the consistent correlation under a t copula, goes through
    q, _ = est.estimate_conditional_probability(lower, upper, given, dof=DOF, corr="quadrant", densities=densities, **small)
    assert np.all((q.prob > 0) & (q.prob < 1))
