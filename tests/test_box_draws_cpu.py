"""CPU tests of the scenarios given a box event (mlmc_copula_box_draws_batch; tool.simple_distribution.copula_box_draws /
event_samples / EventScenarios; Estimate.sample_given_event / estimate_event_means): the NumPy twin of the draws against the
extended-precision reference, its weights against the twin of the box probabilities bit for bit, closed-form conditional means
through the twin with the seeds and n of the GPU tests, the order of the chain, the edge cases, the host methods of EventScenarios
and every argument error of the Python entries.  Nothing here touches the device."""
import types

import numpy as np
import pytest

from tests import box_draw_cases as dc
from tests import box_prob_cases as bc
from tests import joint_sample_cases as jc


def _sd():
    from mlmc_amd.tool import simple_distribution
    return simple_distribution


@pytest.mark.parametrize("case", dc.POINT_CASES, ids=repr)
def test_twin_against_reference(case):
    """z per point and component, in the unit of the cases file; the record there is what this prints"""
    z = dc.case_twin(case)[1]
    worst = dc.worst_z_units(z, case)
    print("twin z against the reference, {}: {:.4g} units (record {})".format(case, worst, dc.TWIN_Z_UNITS_OBSERVED))
    assert worst <= dc.TWIN_Z_UNITS_OBSERVED


def test_tolerance_is_the_record_times_the_margin():
    assert dc.GPU_Z_TOLERANCE_UNITS == dc.TWIN_Z_UNITS_OBSERVED * bc.DEVICE_MARGIN and bc.DEVICE_MARGIN == 16 == jc.z_tolerance()


@pytest.mark.parametrize("case", dc.POINT_CASES + dc.SHAPE_CASES[:4], ids=repr)
def test_weights_are_those_of_the_probability_twin(case):
    """bit for bit on the same points: the draws add operations to the chain, they change none"""
    f = dc.case_twin(case)[0]
    for r, seed in enumerate(case.seeds):
        w = case.w(seed)
        for b in range(case.B):
            want = bc.twin(case.L, case.lo[b], case.hi[b], None if case.shift is None else case.shift[b], w[:case.M - 1])[0]
            assert np.array_equal(f[r, b].view(np.uint64), np.broadcast_to(want, f[r, b].shape).view(np.uint64))


@pytest.mark.parametrize("case", dc.POINT_CASES + dc.SHAPE_CASES, ids=repr)
def test_every_draw_lies_in_its_box(case):
    f, z, u, _ = dc.case_twin(case)
    assert np.all(np.isfinite(z)) and np.all(f >= 0)
    assert np.all(z >= case.lo[None, :, :, None]) and np.all(z <= case.hi[None, :, :, None])
    assert np.all((u >= dc.U_LO) & (u <= dc.U_HI))


@pytest.mark.parametrize("name,lo,hi,comp,exact", dc.closed_form_events(), ids=[c[0] for c in dc.closed_form_events()])
def test_closed_forms_through_the_twin(name, lo, hi, comp, exact):
    res = [dc.twin(dc.L2, lo, hi, None, bc.points(s, [0, 1], 0, bc.CLOSED_N, True)) for s in bc.SEEDS8]
    f, x = np.array([r[0] for r in res]), np.array([r[1][comp] for r in res])
    mean, stderr = dc.ratio_summary(f, x)
    print("{}: {:.8g} exact {:.8g}, {:.2f} stderr".format(name, mean, exact, abs(mean - exact) / stderr))
    assert abs(mean - exact) <= 5 * stderr


def test_closed_form_constants():
    """the probability behind the conditional means: SciPy's bivariate CDF against asin at (0, 0), and against the twin elsewhere"""
    from scipy import stats
    p00 = float(stats.multivariate_normal([0.0, 0.0], [[1.0, bc.RHO2], [bc.RHO2, 1.0]]).cdf([0.0, 0.0]))
    assert abs(p00 - dc.orthant_probability(0.0, 0.0)) < 1e-7
    for h, k in dc.CLOSED_LIMITS[1:]:
        reps = [bc.tree_mean(dc.twin(dc.L2, np.array([h, k]), np.full(2, np.inf), None, bc.points(s, [0, 1], 0, bc.CLOSED_N, True))[0], 0)
                for s in bc.SEEDS8]
        prob, stderr = bc.summary(reps)
        assert abs(prob - dc.orthant_probability(h, k)) <= 5 * stderr + 1e-7 * prob


@pytest.mark.parametrize("perm", [(0, 1, 2), (1, 0, 2), (1, 2, 0), (2, 1, 0)])
def test_constrained_components_go_first(perm):
    """CORR3, only the original component 0 constrained (> 2), the caller's components in the order `perm`: the chain of
    event_samples (`_event_order`, the factor of the permuted correlation) has constant weights, ess = n; with the constrained
    component last in the chain the weights carry the conditioning"""
    sd = _sd()
    perm = np.array(perm)
    corr = bc.CORR3[np.ix_(perm, perm)]                       # the caller's correlation
    c = int(np.flatnonzero(perm == 0)[0])                     # the caller's index of the constrained component
    lo, hi = np.full(3, -np.inf), np.full(3, np.inf)
    lo[c] = 2.0
    order = sd._event_order([c], 3)
    assert order[0] == c and np.array_equal(order[1:], np.setdiff1d(np.arange(3), [c]))
    n = 1024
    w = bc.points(5, [0, 1, 2], 0, n, True)
    f, z, _, _ = dc.twin(sd.correlation_factor(corr[np.ix_(order, order)])[0], lo[order], hi[order], None, w)
    assert np.all(f == f[0]) and abs(dc.ess(f) - n) <= 1e-9 * n
    back = np.empty_like(z)
    back[order] = z                                           # the caller's rows
    assert np.all(back[c] >= 2.0) and np.all(z[0] >= 2.0)
    if tuple(perm[order]) == (0, 1, 2):                       # the same chain as the identity: the same draws, row by row
        z_id = dc.twin(sd.correlation_factor(bc.CORR3)[0], np.array([2.0, -np.inf, -np.inf]), hi, None, w)[1]
        assert np.array_equal(back, z_id[perm])
    last = np.concatenate([order[1:], order[:1]])             # the constrained component at the end of the chain
    f_last = dc.twin(sd.correlation_factor(corr[np.ix_(last, last)])[0], lo[last], hi[last], None, w)[0]
    assert dc.ess(f_last) < 0.5 * n


def test_event_order():
    sd = _sd()
    assert sd._event_order([], 4).tolist() == [0, 1, 2, 3]
    assert sd._event_order([1, 3], 5).tolist() == [1, 3, 0, 2, 4]


@pytest.mark.parametrize("n", [1, 63, 1000])
def test_edge_cases_through_the_twin(n):
    w = bc.points(3, [0, 1, 2], 0, n, True)
    L = bc.chol_factor(3, 11)
    inf = np.full(3, np.inf)
    f, z, u, _ = dc.twin(L, -inf, inf, None, w)
    assert np.all(f == 1.0)                                                                # the full space: plain joint draws
    from scipy import special
    y = special.ndtri(w)
    plain = np.array([y[0] * L[0, 0], L[1, 0] * y[0] + L[1, 1] * y[1], (L[2, 0] * y[0] + L[2, 1] * y[1]) + L[2, 2] * y[2]])
    assert np.all(np.abs(z - plain) <= 8 * bc.U * np.maximum(1.0, np.abs(plain)))
    for lo_e, hi_e in ((np.array([-1.0, 0.3, -1.0]), np.array([1.0, 0.3, 1.0])), (np.array([-1.0, -1.0, 0.5]), np.array([1.0, 1.0, -0.5])),
                       (np.array([0.5, -1.0, -1.0]), np.array([0.5, 1.0, 1.0]))):
        f, z, u, _ = dc.twin(L, lo_e, hi_e, None, w)
        empty = lo_e >= hi_e
        assert np.all(f == 0.0) and not np.any(np.signbit(f)) and np.all(np.isfinite(z))
        assert np.all(z[empty] == hi_e[empty][:, None])                                    # an empty component: z = hi
        assert np.all((z[~empty] >= lo_e[~empty][:, None]) & (z[~empty] <= hi_e[~empty][:, None]))
    f, z, _, _ = dc.twin(L, np.array([-1.0, 40.0, -1.0]), np.array([1.0, 41.0, 1.0]), None, w)
    assert np.all(f == 0.0) and np.all(np.isfinite(z)) and np.all((z[1] >= 40.0) & (z[1] <= 41.0))   # weight 0, still in the box
    # M = 1: one coordinate, weight e - d
    one = dc.twin(np.array([[0.7]]), np.array([-0.2]), np.array([0.9]), np.array([0.1]), w[:1])
    assert np.all(one[0] == special.ndtr((0.9 - 0.1) / 0.7) - special.ndtr((-0.2 - 0.1) / 0.7))
    assert np.all((one[1] >= -0.2) & (one[1] <= 0.9)) and (n == 1 or np.ptp(one[1]) > 0)


# ---- the host methods of EventScenarios -----------------------------------------------------------------------------------------
def _scenarios(draws, weights):
    sd = _sd()
    R, B, M, n = draws.shape
    prob = sd._joint_probability(weights.mean(axis=2), n, np.arange(R, dtype=np.uint64))
    return sd.EventScenarios(draws, weights, prob, dc.ess(weights), np.ones(M, dtype=bool), None)


def test_means_and_weighted_quantiles():
    rng = np.random.default_rng(0)
    R, B, M, n = 4, 3, 2, 50
    x, f = rng.standard_normal((R, B, M, n)), rng.uniform(0.1, 1.0, (R, B, n))
    f[:, 2] = 0.0                                                                          # a box without any weight
    x[:, :, 1] = np.nan                                                                    # a component without mass
    s = _scenarios(x, f)
    mean, stderr = s.means()
    assert mean.shape == (B, M) and stderr.shape == (B, M)
    ratio = np.array([[(f[r, b] * x[r, b, 0]).sum() / f[r, b].sum() for b in range(2)] for r in range(R)])
    assert np.allclose(mean[:2, 0], ratio.mean(axis=0), rtol=1e-13) and np.allclose(stderr[:2, 0], np.std(ratio, axis=0, ddof=1) / 2.0, rtol=1e-12)
    assert np.all(np.isnan(mean[2])) and np.all(np.isnan(mean[:, 1]))
    q = s.weighted_quantiles([0.0, 0.25, 0.5, 1.0, 1.5, np.nan])
    assert q.shape == (B, M, 6) and np.all(np.isnan(q[2])) and np.all(np.isnan(q[:, 1])) and np.all(np.isnan(q[:2, 0, 4:]))
    for b in range(2):
        xs, fs = x[:, b, 0].ravel(), f[:, b].ravel()
        order = np.argsort(xs)
        cum = np.cumsum(fs[order]) / fs.sum()
        assert q[b, 0, 0] == xs.min() and q[b, 0, 3] == xs.max()
        for col, p in ((1, 0.25), (2, 0.5)):
            assert q[b, 0, col] == xs[order][np.argmax(cum >= p)]
    # equal weights: the order statistic
    s1 = _scenarios(np.arange(8.0).reshape(1, 1, 1, 8), np.ones((1, 1, 8)))
    assert s1.weighted_quantiles([0.5])[0, 0, 0] == 3.0 and np.all(np.isnan(s1.means()[1])) and s1.means()[0][0, 0] == 3.5


def test_host_methods_refuse_device_tensors():
    import torch
    s = _scenarios(np.zeros((1, 1, 1, 4)), np.ones((1, 1, 4)))
    s.draws, s.weights = torch.zeros((1, 1, 1, 4), dtype=torch.float64), torch.ones((1, 1, 4), dtype=torch.float64)
    for call in (s.means, lambda: s.weighted_quantiles([0.5])):
        with pytest.raises(ValueError, match="copy"):
            call()


# ---- argument errors: raised before anything touches the device ---------------------------------------------------------------
EYE2 = np.eye(2)


@pytest.mark.parametrize("kw,match", [
    (dict(factor=np.ones((2, 3))), "square"),
    (dict(factor=np.eye(bc.MAX_M + 1), lower=-1.0, upper=1.0), "cap"),
    (dict(factor=np.diag([1.0, 0.0])), "row 1"),
    (dict(lower=[0.0, 0.0, 0.0]), "broadcast"),
    (dict(lower=[[0.0, 0.0], [0.0, np.nan]]), "box 1, component 1"),
    (dict(upper=[np.nan, 1.0]), "box 0, component 0"),
    (dict(shift=[0.0, np.inf]), "shift"),
    (dict(n=0), "n must"),
    (dict(first=2 ** 52), "2\\^52"),
    (dict(seeds=[]), "seed"),
    (dict(seeds=[-1]), "seeds"),
    (dict(seeds=[2 ** 64]), "seeds"),
    (dict(streams=[0]), "streams"),                                            # M of them here, not M - 1
    (dict(streams=[0, 1, 2]), "streams"),
    (dict(streams=[0, -1]), "streams"),
    (dict(streams=[0, 1024]), "1024"),
])
def test_copula_box_draws_argument_errors(kw, match):
    args = dict(factor=EYE2, lower=[-1.0, -1.0], upper=[1.0, 1.0], n=64, seeds=[0, 1])
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        _sd().copula_box_draws(**args)


def _fake(domain=(0.0, 1.0), n_intervals=64, degree=21):
    return types.SimpleNamespace(domain=domain, n_intervals=n_intervals, _gauss_degree=degree)


@pytest.mark.parametrize("kw,match", [
    (dict(distrs=[]), "no distributions"),
    (dict(corr=None), "exactly one"),
    (dict(factor=EYE2), "exactly one"),
    (dict(corr=np.eye(3)), "corr must be"),
    (dict(corr=None, factor=np.ones((3, 1))), "factor"),
    (dict(distrs=[_fake(), _fake(n_intervals=32)]), "same quadrature"),
    (dict(n=0), "n must"),
    (dict(seeds=[]), "seed"),
    (dict(seeds=[2 ** 64]), "seeds"),
    (dict(first=-3), "first"),
    (dict(lower=[0.1, 0.2, 0.3]), "broadcast"),
    (dict(lower=[np.nan, 0.2]), "NaN"),
    (dict(given=[0]), "given"),
    (dict(given={2: 0.5}), "component 2"),
    (dict(given={0: 0.5, 1: 0.5}), "nothing is left"),
    (dict(given={0: 0.5}), "component 0 is given and constrained"),
    (dict(given={1: 0.5}, lower=[0.2, -np.inf], upper=[np.inf, 0.8]), "component 1 is given and constrained"),
    (dict(given={0: [0.5, 0.6]}, lower=np.full((3, 2), -np.inf), upper=np.full((3, 2), np.inf)), "2 sets"),
    (dict(streams=[0]), "streams"),                                            # one per component that is not given
    (dict(streams=[0, 1024]), "1024"),
    (dict(given={0: 0.5}, lower=[-np.inf, 0.2], upper=[np.inf, 0.8], streams=[0, 1]), "streams"),
])
def test_event_samples_argument_errors(kw, match):
    args = dict(distrs=[_fake(), _fake()], lower=[0.2, 0.2], upper=[0.8, 0.8], n=64, seeds=[0, 1], corr=EYE2)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        _sd().event_samples(**args)


@pytest.mark.parametrize("call,kw,match", [
    ("sample_given_event", dict(n=0), "n must"),
    ("sample_given_event", dict(seeds=()), "seed"),
    ("sample_given_event", dict(seeds=[2 ** 64]), "seeds"),
    ("sample_given_event", dict(first=-1), "first"),
    ("sample_given_event", dict(lower=[np.nan, 0.0]), "NaN"),
    ("sample_given_event", dict(corr="pearson"), "corr must be"),
    ("estimate_event_means", dict(upper=[np.nan, 0.0]), "NaN"),
    ("estimate_event_means", dict(n=-4), "n must"),
    ("estimate_event_means", dict(seeds=[0.5]), "seeds"),
    ("estimate_event_means", dict(corr="x"), "corr must be"),
])
def test_estimate_argument_errors(call, kw, match):
    from mlmc_amd.estimator import Estimate
    est = Estimate(None, None, None)
    args = dict(lower=[0.0, 0.0], upper=[1.0, 1.0])
    if call == "sample_given_event":
        args["n"] = 64
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        getattr(est, call)(**args)
