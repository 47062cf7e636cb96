"""CPU tests of the t box entries with a conditioned lead component: the NumPy twin of the header's steps
against the tabulated references (down to marginal levels of 1e-12), against SciPy's multivariate t and against `bivariate_t_orthant`;
the choice of the lead and the permutation round trip of `joint_probabilities` / `event_samples` with the device call stubbed; the
argument errors; and that mixing="plain" calls exactly what it has always called.  Nothing here touches a device."""
import numpy as np
import pytest
from scipy import special

from mlmc_amd import estimator
from mlmc_amd.tool import simple_distribution as sd
from tests import box_prob_cases as bc
from tests import t_lead_cases as tl

ABS = 1e-13


def _orthant(kind, M, dof, level):
    L = np.eye(M) if kind == "I" else bc.equicorrelation_factor(M)
    if level == "box":
        return L, np.full(M, tl.TWO_SIDED[0]), np.full(M, tl.TWO_SIDED[1])
    return L, np.full(M, tl.t_upper_quantile(dof, level)), np.full(M, np.inf)


@pytest.mark.parametrize("key", sorted(tl.TWIN, key=repr), ids=lambda k: "-".join(str(x) for x in k))
def test_twin_against_the_references(key):
    kind, M, dof, level = key
    L, lo, hi = _orthant(kind, M, dof, level)
    rep, _ = tl.twin_replicates(L, lo, hi, dof, tl.CLOSED_SEEDS, tl.CLOSED_N)
    prob, stderr = bc.summary(rep)
    exact = (tl.INDEPENDENT if kind == "I" else tl.EQUI)[(M, dof, level)]
    print("{}: twin {:.9g}, exact {:.9g}, off by {:.2f} stderr, rel. stderr {:.3g}".format(key, prob, exact, abs(prob - exact) / stderr,
                                                                                        stderr / prob))
    assert abs(prob - exact) <= 6.0 * stderr + ABS
    # the record that the GPU tests cap the device's standard error with
    rec_prob, rec_rel = tl.TWIN[key]
    assert abs(prob - rec_prob) <= 1e-9 * rec_prob and abs(stderr / prob - rec_rel) <= 1e-6 * rec_rel


def test_relative_error_does_not_grow_with_depth():
    """where the lead carries the box (M = 2, 3 at nu = 3) the relative standard error at level 1e-12 is that at 1e-3 within a factor
    1.1, and the values are right to 1e-4 relative; plain mixing on the same kind of points has lost the box at 1e-6 already"""
    for kind, M in (("I", 2), ("equi", 2), ("equi", 3)):
        rel = [tl.TWIN[(kind, M, 3.0, q)][1] for q in tl.LEVELS]
        assert rel[-1] <= 1.1 * rel[0] and max(rel) < 1e-4
        for q in tl.LEVELS:
            exact = (tl.INDEPENDENT if kind == "I" else tl.EQUI)[(M, 3.0, q)]
            assert abs(tl.TWIN[(kind, M, 3.0, q)][0] - exact) <= 1e-4 * exact
    L, lo, hi = _orthant("equi", 3, 3.0, 1e-6)
    plain = tl.plain_twin_orthant(L, lo, hi, 3.0, tl.CLOSED_SEEDS, tl.CLOSED_N)
    prob, stderr = bc.summary(plain)
    print("plain mixing at 1e-6: seeds {} against {:.6g}".format(np.array2string(plain, precision=2), tl.EQUI[(3, 3.0, 1e-6)]))
    # one or two seeds carry the mean and most are orders of magnitude below the value: nothing is resolved
    assert stderr > 0.5 * prob and np.median(plain) < 1e-3 * tl.EQUI[(3, 3.0, 1e-6)]


def test_reference_functions_reproduce_the_tables():
    assert abs(float(tl.independent_reference(2, 3.0, tl.t_upper_quantile(3.0, 1e-6), np.inf)) - tl.INDEPENDENT[(2, 3.0, 1e-6)]) \
        <= 1e-14 * tl.INDEPENDENT[(2, 3.0, 1e-6)]
    got = tl.equicorrelated_reference(3, 3.0, tl.t_upper_quantile(3.0, 1e-3))
    assert abs(got - tl.EQUI[(3, 3.0, 1e-3)]) <= 1e-12 * got
    # nu = 1 in closed form: two independent-factor Cauchy components beyond t, P -> q (1 - 1 / sqrt(2)) as q -> 0
    assert abs(tl.INDEPENDENT[(2, 1.0, 1e-12)] / 1e-12 - (1.0 - np.sqrt(0.5))) < 1e-9


def test_twin_against_scipy_multivariate_t():
    from scipy.stats._qmvnt import _qmvt
    dof, lo, hi = 3.0, np.array([-0.5, -np.inf, -1.0]), np.array([np.inf, 0.5, 0.6])
    L = np.linalg.cholesky(bc.CORR3)
    for qmc in (False, True):
        rep, _ = tl.twin_replicates(L, lo, hi, dof, bc.SEEDS8, 2 ** 12, qmc=qmc)
        prob, stderr = bc.summary(rep)
        want, abseps, _ = _qmvt(200000, dof, bc.CORR3, lo, hi, np.random.default_rng(0))
        print("twin {:.6f} +- {:.2g}, SciPy {:.6f} +- {:.2g}".format(prob, stderr, want, abseps))
        assert abs(prob - want) <= 6.0 * stderr + abseps


@pytest.mark.parametrize("dof", tl.DOFS)
@pytest.mark.parametrize("rho", [-0.5, 0.7])
def test_twin_against_the_bivariate_orthant(dof, rho):
    L = np.linalg.cholesky(np.array([[1.0, rho], [rho, 1.0]]))
    for level in (0.9, 0.99):
        h = float(sd.t_scores(special.ndtri(level), dof))
        rep, _ = tl.twin_replicates(L, np.array([h, h]), np.full(2, np.inf), dof, bc.SEEDS8, 2 ** 12)
        prob, stderr = bc.summary(rep)
        assert abs(prob - sd.bivariate_t_orthant(h, h, rho, dof)) <= 6.0 * stderr + ABS, (dof, rho, level)


def test_twin_draws_lie_inside_and_empty_lead():
    L = bc.chol_factor(3, 5)
    lo, hi = np.array([2.0, -1.0, -np.inf]), np.array([3.0, np.inf, 0.5])
    p0, w = tl.points_of(3, 3, 0, 256, True, draws=True)
    f, v, sc, z = tl.lead_twin(L, lo, hi, 3.0, p0, w, draws=True)
    assert np.all((z >= lo[:, None]) & (z <= hi[:, None])) and np.all(f > 0) and np.all(sc > 0)
    assert np.array_equal(tl.lead_twin(L, lo, hi, 3.0, p0, w)[0], f)                        # the weights of the probability entry
    f0 = tl.lead_twin(L, np.array([0.5, -1.0, -1.0]), np.array([-0.5, 1.0, 1.0]), 3.0, p0, w)[0]
    assert np.all(f0 == 0.0)


# ---- the choice of the lead and the round trip, the device call stubbed ---------------------------------------------------------------
class _Flat:
    """a distribution on (0, 1) as far as the host code of the box entries looks"""
    domain = (0.0, 1.0)


def test_lead_components():
    lo = np.array([[1.0, 2.0, -np.inf], [-np.inf, -np.inf, -np.inf], [0.5, 0.5, 0.5], [-3.0, 1.0, 5.0]])
    hi = np.array([[np.inf, np.inf, np.inf], [0.0, -4.0, np.inf], [np.inf, np.inf, np.inf], [3.0, np.inf, 4.0]])
    lead, marg = sd.lead_components(lo, hi, 3.0)
    assert lead.tolist() == [1, 1, 0, 2]                 # the rarest; a tie goes to the lowest index; an empty component has mass 0
    assert marg[3, 2] == 0.0 and marg[1, 2] == 1.0
    # an upper-tail pair keeps its relative accuracy: through the lower tail of the mirrored limits
    far = sd.lead_components(np.array([[1e8, 1e8 * (1 + 1e-9)]]), np.array([[np.inf, np.inf]]), 3.0)
    assert far[0].tolist() == [1] and far[1][0, 1] < far[1][0, 0]
    assert sd.lead_components(lo, hi, 3.0, candidates=[0, 2])[0].tolist() == [0, 0, 0, 2]


def _stub_scores(monkeypatch):
    """limits in (0, 1) of the flat distributions map to normal scores without the device"""
    monkeypatch.setattr(sd, "_common_quadrature", lambda what, distrs: None)
    monkeypatch.setattr(sd, "_domain_arrays", lambda distrs: (np.zeros(len(distrs)), np.ones(len(distrs))))
    monkeypatch.setattr(sd, "normal_scores", lambda distrs, x: special.ndtri(np.asarray(x)))


CORR4 = np.array([[1.0, 0.5, 0.2, 0.1], [0.5, 1.0, 0.3, -0.2], [0.2, 0.3, 1.0, 0.4], [0.1, -0.2, 0.4, 1.0]])


def test_joint_probabilities_groups_by_lead(monkeypatch):
    _stub_scores(monkeypatch)
    calls = []

    def fake(factor, lower, upper, n, seeds, **kw):
        calls.append((np.array(factor), np.array(lower), np.array(upper), kw))
        B = np.shape(lower)[0]
        rep = np.arange(len(seeds) * B, dtype=np.float64).reshape(len(seeds), B) + 100.0 * len(calls)
        res = sd._joint_probability(rep, n, np.asarray(seeds, dtype=np.uint64))
        return (res, np.full((len(seeds), B, n), float(len(calls)))) if kw.get("return_integrand") else res
    monkeypatch.setattr(sd, "copula_box_probabilities", fake)
    distrs = [_Flat() for _ in range(4)]
    # component 1 is never constrained; box 0: component 3 is the rarest, box 1: component 0, box 2: component 3
    lower = np.array([[0.9, 0.0, 0.99, 0.999], [0.9999, 0.0, 0.5, 0.9], [0.0, 0.0, 0.0, 0.0]])
    upper = np.array([[1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0], [0.9, 1.0, 0.5, 0.01]])
    res, f = sd.joint_probabilities(distrs, lower, upper, 64, [1, 2], corr=CORR4, dof=3.0, mixing="conditioned", return_integrand=True)
    assert len(calls) == 2
    keep = np.array([0, 2, 3])
    seen = {}
    for k, (factor, lo, hi, kw) in enumerate(calls):
        assert kw["mixing"] == "conditioned" and kw["dof"] == 3.0
        # which permutation of the kept components reproduces the factor's correlation
        order = next(p for p in ([0, 2, 3], [2, 0, 3], [3, 0, 2]) if np.allclose(factor @ factor.T, CORR4[np.ix_(p, p)], atol=1e-12))
        seen[order[0]] = (k, lo.shape[0])
        assert order[1:] == sorted(order[1:])             # the others keep their order
        t_lo = sd.t_scores(special.ndtri(np.clip(lower[:, order], 1e-300, 1.0)), 3.0)
        boxes = [0, 2] if order[0] == 3 else [1]
        finite = np.isfinite(lo)
        assert np.allclose(lo[finite], t_lo[boxes][finite])
    assert seen == {0: (0, 1), 3: (1, 2)}                  # groups ascending in the lead; box 1 alone, boxes 0 and 2 together
    # replicates and the integrand are back in the order of the boxes
    assert res.replicates[:, 1].tolist() == [100.0, 101.0] and res.replicates[:, [0, 2]].tolist() == [[200.0, 201.0], [202.0, 203.0]]
    assert np.all(f[:, 1] == 1.0) and np.all(f[:, [0, 2]] == 2.0)
    # the rarest component first in the caller's order: one group, nothing to permute
    calls.clear()
    sd.joint_probabilities(distrs[:2], [[0.999, 0.9]], 1.0, 64, [1], corr=CORR4[:2, :2], dof=3.0, mixing="conditioned")
    assert len(calls) == 1 and np.allclose(calls[0][0] @ calls[0][0].T, CORR4[:2, :2])


def test_event_samples_round_trip(monkeypatch):
    _stub_scores(monkeypatch)
    calls = []

    def fake(factor, lower, upper, n, seeds, **kw):
        calls.append((np.array(factor), kw))
        B, M, R = np.shape(lower)[0], np.shape(lower)[1], len(seeds)
        # row i of u holds the marginal level that identifies the component at chain position i through its correlations
        order = next(list(p) for p in __import__("itertools").permutations(range(4))
                     if np.allclose(factor @ factor.T, CORR4[np.ix_(p, p)], atol=1e-12))
        u = np.empty((R, B, M, n))
        for i, m in enumerate(order):
            u[:, :, i, :] = (m + 1) / 10.0
        rep = np.full((R, B), 0.25)
        return sd.BoxDraws(u.copy(), u, np.ones((R, B, n)), sd._joint_probability(rep, n, np.asarray(seeds, dtype=np.uint64)))
    monkeypatch.setattr(sd, "copula_box_draws", fake)
    monkeypatch.setattr(sd, "_on_rule", lambda chain, pts, *a: ([10.0 * p for p in pts], np.ones(len(chain))))
    distrs = [_Flat() for _ in range(4)]
    lower = np.array([[0.9, 0.0, 0.99, 0.999], [0.9999, 0.0, 0.5, 0.9]])
    scen = sd.event_samples(distrs, lower, 1.0, 8, [1, 2], corr=CORR4, dof=3.0, mixing="conditioned")
    assert len(calls) == 2 and all(kw["mixing"] == "conditioned" for _, kw in calls)
    # rows come back in the components' own order whatever the lead was
    for m in range(4):
        assert np.all(scen.uniforms[:, :, m, :] == (m + 1) / 10.0) and np.all(scen.draws[:, :, m, :] == (m + 1.0))
    assert scen.weights.shape == (2, 2, 8) and np.all(scen.prob.replicates == 0.25)


# ---- the argument errors, and plain mixing -------------------------------------------------------------------------------------------
def _box(fn, **kw):
    return fn(np.eye(3), [-1.0] * 3, [1.0] * 3, 64, [0], **kw)


@pytest.mark.parametrize("fn", [sd.copula_box_probabilities, sd.copula_box_draws], ids=["probabilities", "draws"])
def test_argument_errors_of_the_score_entries(fn):
    with pytest.raises(ValueError, match='mixing must be "plain" or "conditioned"'):
        _box(fn, dof=3, mixing="lead")
    with pytest.raises(ValueError, match='mixing="conditioned" needs dof'):
        _box(fn, mixing="conditioned")
    with pytest.raises(ValueError, match='mixing="conditioned" needs dof'):
        _box(fn, dof=np.inf, mixing="conditioned")
    with pytest.raises(ValueError, match="together with shift"):
        _box(fn, dof=3, shift=np.zeros(3), mixing="conditioned")
    with pytest.raises(ValueError, match='return_lead needs mixing="conditioned"'):
        _box(fn, dof=3, return_lead=True)
    with pytest.raises(ValueError, match="mix_stream 2 is the stream of"):
        _box(fn, dof=3, mix_stream=2, mixing="conditioned")
    with pytest.raises(ValueError, match="dof must lie in"):
        _box(fn, dof=65.0, mixing="conditioned")


def test_argument_errors_of_the_entries_in_own_units():
    two = [object()] * 2
    with pytest.raises(ValueError, match='mixing="conditioned" together with given'):
        sd._check_mixing("joint_probabilities", "conditioned", 3.0, None, {0: 0.1})
    for fn in (sd.joint_probabilities, sd.event_samples):
        with pytest.raises(ValueError, match="dof together with given"):                    # the older check comes first
            fn(two, -np.inf, 0.0, 64, [0], corr=np.eye(2), dof=3, given={0: 0.1}, mixing="conditioned")
        with pytest.raises(ValueError, match='mixing="conditioned" needs dof'):
            fn(two, -np.inf, 0.0, 64, [0], corr=np.eye(2), mixing="conditioned")
        with pytest.raises(ValueError, match="mixing must be"):
            fn(two, -np.inf, 0.0, 64, [0], corr=np.eye(2), dof=3, mixing=True)


class _NoWalk(estimator.Estimate):
    def __init__(self):
        pass


def test_estimate_argument_errors():
    est = _NoWalk()
    calls = (lambda **kw: est.estimate_joint_probability(-np.inf, 0.0, corr=np.eye(2), **kw),
             lambda **kw: est.estimate_joint_exceedance(0.0, corr=np.eye(2), **kw),
             lambda **kw: est.sample_given_event(64, -np.inf, 0.0, corr=np.eye(2), **kw),
             lambda **kw: est.estimate_event_means(-np.inf, 0.0, corr=np.eye(2), **kw),
             lambda **kw: est.estimate_aggregates(weights=[1.0, 1.0], event=(-np.inf, 0.0), corr=np.eye(2), **kw))
    for call in calls:
        with pytest.raises(ValueError, match='mixing="conditioned" needs dof'):
            call(mixing="conditioned")
        with pytest.raises(ValueError, match="mixing must be"):
            call(dof=3, mixing="other")
    with pytest.raises(ValueError, match='mixing="conditioned" needs event'):
        est.estimate_aggregates(weights=[1.0, 1.0], corr=np.eye(2), dof=3, mixing="conditioned")
    # the bootstrap bands and the conditional family have no such keyword: they keep plain mixing
    import inspect
    for name in ("bootstrap_joint_probability", "bootstrap_joint_exceedance", "estimate_conditional_probability",
                 "estimate_conditional_exceedance", "sample_conditional_event", "estimate_conditional_event_means",
                 "estimate_conditional_aggregates"):
        assert "mixing" not in inspect.signature(getattr(estimator.Estimate, name)).parameters, name


class _Recorder:
    """stands in for the loaded library: records the entry called and its arguments, returns success"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


def test_plain_mixing_calls_what_it_always_called(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(sd._lib, "lib", lambda: rec)
    monkeypatch.setattr(sd._lib, "check", lambda rc: None)
    L = np.linalg.cholesky(bc.CORR3)
    lo, hi = [-1.0] * 3, [1.0] * 3
    for kw in (dict(), dict(mixing="plain")):
        rec.calls.clear()
        sd.copula_box_probabilities(L, lo, hi, 64, [0], dof=3.0, return_mixing=True, **kw)
        sd.copula_box_draws(L, lo, hi, 64, [0], dof=3.0, **kw)
        sd.copula_box_probabilities(L, lo, hi, 64, [0], **kw)
        names = [c[0] for c in rec.calls]
        assert names == ["mlmc_copula_box_prob_t_batch", "mlmc_copula_box_draws_t_batch", "mlmc_copula_box_prob_batch"]
        assert len(rec.calls[0][1]) == 17 and len(rec.calls[1][1]) == 19                    # the arguments of the t entries, no more
        assert rec.calls[0][1][9] == 0 and rec.calls[0][1][5] == 3.0                        # mix_stream 0, dof
    rec.calls.clear()
    sd.copula_box_probabilities(L, lo, hi, 64, [0], dof=3.0, mixing="conditioned", return_lead=True)
    sd.copula_box_draws(L, lo, hi, 64, [0], dof=3.0, mixing="conditioned")
    assert [c[0] for c in rec.calls] == ["mlmc_copula_box_prob_tl_batch", "mlmc_copula_box_draws_tl_batch"]
    assert len(rec.calls[0][1]) == 18 and len(rec.calls[1][1]) == 20


def test_abi_names_the_new_entries():
    import os
    import re
    from mlmc_amd import _lib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mlmc_hip.h")).read()
    head = text.split("#define MLMC_ABI_VERSION")[1].split("*/")[0]
    for name in ("mlmc_copula_box_prob_tl_batch", "mlmc_copula_box_draws_tl_batch"):
        assert name in head and name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert re.search(r"#define\s+MLMC_ABI_VERSION\s+8\b", text) and _lib.ABI_VERSION == 8
