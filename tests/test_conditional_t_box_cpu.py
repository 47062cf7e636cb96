"""CPU tests of the conditional box probabilities and event scenarios under the Student-t copula: the NumPy twin against closed
forms and SciPy's multivariate t, the host algebra (mu, r and the factor of the reduced problem) against the block formulas, and the
argument checks of every new entry, all raised before anything touches the device.  Nothing here touches a device."""
import numpy as np
import pytest
from scipy import integrate, special, stats

from mlmc_amd import _lib, estimator
from mlmc_amd.tool import simple_distribution as sd
from tests import box_prob_cases as bc
from tests import conditional_t_box_cases as ctc
from tests import t_box_cases as tb


@pytest.fixture
def no_device(monkeypatch):
    def forbidden(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(_lib, "lib", forbidden)
    monkeypatch.setattr(_lib, "init", forbidden)


def test_twin_is_the_t_twin_on_the_shifted_and_scaled_limits():
    """point by point ct_twin is tests/box_prob_cases.twin on the limits (lo - shift) / (scale s_j), bit for bit; an empty
    component gives exactly 0; zero shift and unit scale give t_twin itself"""
    L, lo, hi, shift, scale = ctc.problem(3, 4)
    s = np.sqrt(4.0 / stats.chi2.ppf(tb.mixing_points(5, 37, 24, False), 4.0))
    w = bc.points(5, tb.chain_streams(3), 37, 24, False)
    for b in range(4):
        f = ctc.ct_twin(L, lo[b], hi[b], shift[b], scale[b], s, w)
        lt, ht = ctc.scaled_limits(lo[b], hi[b], shift[b], scale[b], s)
        for j in range(s.size):
            want, _ = bc.twin(L, lt[j], ht[j], None, w[:, j:j + 1])
            assert np.array_equal(f[j:j + 1].view(np.uint64), want.view(np.uint64))
        assert np.array_equal(ctc.ct_twin(L, lo[b], hi[b], np.zeros(3), 1.0, s, w).view(np.uint64),
                              tb.t_twin(L, lo[b], hi[b], s, w).view(np.uint64))
    assert np.all(ctc.ct_twin(L, lo[3], hi[3], shift[3], scale[3], s, w) == 0.0)
    assert np.all(np.isinf(ctc.scaled_limits(lo[1], hi[1], shift[1], scale[1], s)[1]))      # infinite limits stay infinite
    assert np.all(shift != 0) and np.all((scale > 0.3) & (scale < 4.0))


def test_recorded_reference_of_the_two_component_case():
    """(b): dblquad of SciPy's multivariate t density over the box, against the recorded value"""
    law = ctc.LAWS[1]
    dist = stats.multivariate_t(loc=law.mu, shape=law.r ** 2 * law.sigma, df=law.dof_mix)
    # y_2 in (-inf, 1) outside, y_1 in (0.5, inf) inside
    got, err = integrate.dblquad(lambda y1, y2: dist.pdf([y1, y2]), -np.inf, 1.0, 0.5, np.inf, epsabs=1e-11, epsrel=1e-11)
    print("dblquad {:.11f} +- {:.1g}, recorded {:.11f}".format(got, err, ctc.DBLQUAD_B))
    assert err < 1e-9 and abs(got - ctc.DBLQUAD_B) <= 1e-9
    # E[T_nu(Y_m) | box, given], the event means under uniform marginals
    for k, want in enumerate(ctc.EVENT_MEANS_B):
        num, err = integrate.dblquad(lambda y1, y2: stats.t.cdf((y1, y2)[k], law.dof) * dist.pdf([y1, y2]), -np.inf, 1.0, 0.5, np.inf,
                                     epsabs=1e-10, epsrel=1e-10)
        print("E[X_{} | box, given] {:.12f} +- {:.1g}, recorded {:.12f}".format(k + 1, num / got, err / got, want))
        assert err < 1e-9 and abs(num / got - want) <= 1e-9


@pytest.mark.parametrize("law", ctc.LAWS, ids=repr)
def test_twin_against_the_references(law):
    """the gate on the inputs of the GPU tests: the twin's mean over 8 seeds of 2^12 Sobol' points within 3 of its own standard
    errors of the reference"""
    exact = law.reference()
    prob, stderr = law.twin_mean()
    print("{}: twin {:.10f} +- {:.2g}, reference {:.10f}, off by {:.2f} standard errors; r = {:.4f}".format(
        law.name, prob, stderr, exact, abs(prob - exact) / stderr, law.r))
    assert 0.01 < exact < 0.99 and stderr > 0
    assert abs(prob - exact) <= 3.0 * stderr
    if law.name == "eye":
        # under the Gaussian copula the given value changes nothing: the unconditional normal probability, far from the t one
        gauss = special.ndtr(special.ndtri(stats.t.cdf(2.0, law.dof))) - special.ndtr(special.ndtri(stats.t.cdf(-1.0, law.dof)))
        assert law.r > 1.5 and abs(gauss - exact) > 0.1


@pytest.mark.parametrize("observed, keep", [((1,), (0, 2)), ((0, 3), (1,)), ((2,), (0,))])
def test_host_algebra_against_the_block_formulas(observed, keep):
    """mu = C_UO C_OO^-1 y_O, r^2 = (nu + y_O^T C_OO^-1 y_O) / (nu + p) and the Schur complement restricted to `keep`, a strict
    subset of the components that are not given: what conditional_probabilities hands to the score entry"""
    rng = np.random.default_rng(11)
    a = rng.standard_normal((4, 9))
    corr = a @ a.T
    d = 1.0 / np.sqrt(np.diag(corr))
    corr = corr * d[:, None] * d[None, :]
    dof = 3.0
    y_obs = rng.standard_normal((len(observed), 2)) * 2.0
    w, fc, info, l_oo = sd.conditional_factor(corr, observed, return_observed=True)
    mu = (w @ y_obs).T
    r = sd._conditional_t_scale(y_obs, l_oo, dof)
    keep = np.asarray(keep)
    assert keep.size < info.unobserved.size
    low = np.linalg.cholesky((fc @ fc.T)[np.ix_(keep, keep)])
    for b in range(2):
        un, mu_b, r_b, sigma = ctc.block_law(corr, observed, y_obs[:, b], dof)
        assert np.array_equal(un, info.unobserved)
        np.testing.assert_allclose(mu[b], mu_b, rtol=0, atol=1e-12)
        np.testing.assert_allclose(r[b], r_b, rtol=1e-13)
        np.testing.assert_allclose(low @ low.T, sigma[np.ix_(keep, keep)], rtol=0, atol=1e-12)
        assert np.all(np.diag(low) > 0) and np.all(np.triu(low, 1) == 0)


# ---- argument errors, all before any device call -------------------------------------------------------------------------------------
def _box(fn, **kw):
    kw.setdefault("dof", 3)
    return fn(np.eye(3), [-1.0] * 3, [1.0] * 3, 64, [0], **kw)


@pytest.mark.parametrize("fn", [sd.conditional_box_probabilities, sd.conditional_box_draws], ids=["probabilities", "draws"])
def test_argument_errors_of_the_score_entries(no_device, fn):
    for bad in (0.5, 192.5, np.nan, True, "many", np.inf):
        with pytest.raises(ValueError, match="dof_mix must lie in"):
            _box(fn, dof_mix=bad)
    for bad in (0.5, 65.0, np.nan, None, np.inf):
        with pytest.raises(ValueError, match="dof must"):
            _box(fn, dof=bad)
    for bad in (0.0, -1.0, np.inf, np.nan, [1.0, 0.0, 1.0]):
        with pytest.raises(ValueError, match="scale"):
            _box(fn, scale=bad)
    with pytest.raises(ValueError, match="shift must be finite"):
        _box(fn, shift=[0.0, np.inf, 0.0])
    with pytest.raises(ValueError, match="does not broadcast"):
        _box(fn, shift=np.zeros(2))
    count = 2 if fn is sd.conditional_box_probabilities else 3
    with pytest.raises(ValueError, match="mix_stream must be given"):
        _box(fn, streams=list(range(4, 4 + count)))
    with pytest.raises(ValueError, match="mix_stream 2 is the stream of"):
        _box(fn, mix_stream=2)
    with pytest.raises(ValueError, match="below 1024"):
        _box(fn, mix_stream=1024)


def test_existing_entries_still_raise(no_device):
    for fn in (sd.copula_box_probabilities, sd.copula_box_draws):
        with pytest.raises(ValueError, match="dof together with shift.*conditional_box_"):
            fn(np.eye(3), [-1.0] * 3, [1.0] * 3, 64, [0], dof=3, shift=np.zeros(3))
    two = [object()] * 2
    for fn, name in ((sd.joint_probabilities, "joint_probabilities"), (sd.event_samples, "event_samples")):
        with pytest.raises(ValueError, match="^" + name + ": dof together with given.*conditional_"):
            fn(two, -np.inf, 0.0, 64, [0], corr=np.eye(2), dof=3, given={0: 0.1})
    with pytest.raises(ValueError, match="dof together with given.*conditional_aggregates"):
        sd.joint_aggregates(two, 4, 1, corr=np.eye(2), dof=3, given={0: 0.1})


def test_argument_errors_of_the_entries_in_own_units(no_device):
    many = [object()] * 131
    given = {k: 0.1 for k in range(129)}                                                   # 64 + 129 > 192
    eye = np.eye(131)
    for call in (lambda **kw: sd.conditional_probabilities(many, -np.inf, 0.0, n=64, seeds=[0], corr=eye, **kw),
                 lambda **kw: sd.conditional_event_samples(many, -np.inf, 0.0, n=64, seeds=[0], corr=eye, **kw),
                 lambda **kw: sd.conditional_aggregates(many, 4, 1, corr=eye, **kw)):
        with pytest.raises(ValueError, match="exceeds 192"):
            call(given=given, dof=64)
        with pytest.raises(ValueError, match="given is required"):
            call(given=None, dof=3)
        with pytest.raises(ValueError, match="dof must lie in"):
            call(given={0: 0.1}, dof=0.5)
        with pytest.raises(ValueError, match="mix_stream needs dof"):
            call(given={0: 0.1}, mix_stream=3)


def test_a_given_component_must_not_be_constrained(monkeypatch):
    """conditional_event_samples takes limits over ALL components: a limit on a given one is an error before any device call (the
    domains come from a stub, the first device call would be normal_scores)"""
    def forbidden(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(sd, "normal_scores", forbidden)
    monkeypatch.setattr(sd, "_common_quadrature", lambda what, distrs: (0, 0))
    monkeypatch.setattr(sd, "_domain_arrays", lambda distrs: (np.zeros(len(distrs)), np.ones(len(distrs))))
    three = [object()] * 3
    with pytest.raises(ValueError, match="component 1 is given and constrained"):
        sd.conditional_event_samples(three, [0.2, 0.3, -np.inf], np.inf, {1: 0.5}, 64, [0], corr=np.eye(3), dof=3)
    # a call that constrains nothing returns ones without a device call
    res = sd.conditional_probabilities(three, -np.inf, np.inf, {1: 0.5}, 64, [0, 1], corr=np.eye(3), dof=3)
    assert np.array_equal(res.replicates, np.ones((2, 1))) and res.prob[0] == 1.0
    res, f = sd.conditional_probabilities(three, -np.inf, np.inf, {1: 0.5}, 64, [0, 1], corr=np.eye(3), dof=3, return_integrand=True)
    assert f is None and res.prob[0] == 1.0


class _NoWalk(estimator.Estimate):
    """an Estimate whose quantity must not be touched: the checks under test come first"""

    def __init__(self):
        pass


def test_estimate_argument_errors(no_device):
    est = _NoWalk()
    given = {k: 0.1 for k in range(129)}
    calls = (lambda **kw: est.estimate_conditional_probability(-np.inf, 0.0, corr=np.eye(2), **kw),
             lambda **kw: est.estimate_conditional_exceedance(0.0, corr=np.eye(2), **kw),
             lambda **kw: est.sample_conditional_event(64, -np.inf, 0.0, corr=np.eye(2), **kw),
             lambda **kw: est.estimate_conditional_event_means(-np.inf, 0.0, corr=np.eye(2), **kw))
    for call in calls:
        for bad in (0.5, 100.0, np.nan):
            with pytest.raises(ValueError, match="dof must lie in"):
                call(given={0: 0.1}, dof=bad)
        with pytest.raises(ValueError, match="exceeds 192"):
            call(given=given, dof=64)
        with pytest.raises(ValueError, match="given is required"):
            call(given=None)
    with pytest.raises(ValueError, match="given is required"):
        est.estimate_conditional_aggregates(None)
    # the existing methods keep their errors and name the new ones
    with pytest.raises(ValueError, match="dof together with given.*conditional"):
        est.estimate_joint_probability(-np.inf, 0.0, corr=np.eye(2), dof=3, given={0: 0.1})
    with pytest.raises(ValueError, match="dof together with given.*conditional"):
        est.sample_given_event(64, -np.inf, 0.0, corr=np.eye(2), dof=3, given={0: 0.1})
