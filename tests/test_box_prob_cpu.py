"""CPU tests of the joint box probabilities (mlmc_copula_box_prob_batch; tool.simple_distribution.copula_box_probabilities /
joint_probabilities; Estimate.estimate_joint_probability / estimate_joint_exceedance): the NumPy twin of the integrand against
the extended-precision reference, the closed forms and exact cases through the twin with the seeds and n of the GPU tests, and
every argument error of the Python entries.  Nothing here touches the device."""
import types

import numpy as np
import pytest
from scipy import special

from tests import box_prob_cases as bc
from tests import joint_sample_cases as jc


@pytest.mark.parametrize("case", bc.POINT_CASES, ids=repr)
def test_twin_against_reference(case):
    """per point, in the unit of the cases file; the record there is what this prints"""
    f, scale = bc.case_twin(case)
    ref = bc.case_reference(case)
    worst = max(float(bc.units(f[r, b], ref[r][b], scale[r, b]).max()) for r in range(len(case.seeds)) for b in range(case.B))
    print("twin against the reference, {}: {:.4g} units (record {})".format(case, worst, bc.TWIN_UNITS_OBSERVED))
    assert worst <= bc.TWIN_UNITS_OBSERVED
    # the mean through the tree against the reference mean: the points' errors and n roundings of the sum
    for r in range(len(case.seeds)):
        for b in range(case.B):
            want = float(bc.reference_mean(ref[r][b]))
            got = bc.tree_mean(f[r, b], case.first, case.M)
            assert abs(got - want) <= bc.U * (bc.TWIN_UNITS_OBSERVED * scale[r, b].max() + case.n) * want


def test_tolerance_is_the_record_times_the_margin():
    assert bc.GPU_TOLERANCE_UNITS == bc.TWIN_UNITS_OBSERVED * bc.DEVICE_MARGIN and bc.DEVICE_MARGIN == jc.z_tolerance()


@pytest.mark.parametrize("name,L,lo,hi,exact", bc.closed_forms(), ids=[c[0] for c in bc.closed_forms()])
def test_closed_forms_through_the_twin(name, L, lo, hi, exact):
    M = L.shape[0]
    reps = [bc.tree_mean(bc.twin(L, lo, hi, None, bc.points(s, list(range(M - 1)), 0, bc.CLOSED_N, True))[0], 0) for s in bc.SEEDS8]
    prob, stderr = bc.summary(reps)
    print("{}: {:.10g} exact {:.10g}, {:.2f} stderr".format(name, prob, exact, abs(prob - exact) / stderr))
    assert abs(prob - exact) <= 5 * stderr


@pytest.mark.parametrize("n", [1, 63, 1000])
def test_exact_cases_through_the_twin(n):
    w = bc.points(3, [0, 1], 0, n, True)
    eye = np.eye(3)
    lo, hi = np.array([-1.0, 0.5, -np.inf]), np.array([0.25, np.inf, 1.5])
    f, _ = bc.twin(eye, lo, hi, None, w)
    widths = [special.ndtr(0.25) - special.ndtr(-1.0), special.ndtr(-0.5) - special.ndtr(-np.inf), special.ndtr(1.5) - 0.0]
    assert np.all(f == 1.0 * widths[0] * widths[1] * widths[2])                          # independent components: any n
    L = bc.chol_factor(3, 11)
    inf = np.full(3, np.inf)
    assert np.all(bc.twin(L, -inf, inf, None, w)[0] == 1.0) and bc.tree_mean(bc.twin(L, -inf, inf, None, w)[0], 0) == 1.0
    for lo_e, hi_e in ((np.array([-1.0, 0.3, -1.0]), np.array([1.0, 0.3, 1.0])), (np.array([-1.0, -1.0, 0.5]), np.array([1.0, 1.0, -0.5])),
                       (np.array([np.inf, -1.0, -1.0]), inf)):
        f = bc.twin(L, lo_e, hi_e, None, w)[0]
        assert np.all(f == 0.0) and not np.any(np.signbit(f))                              # an empty box
    f = bc.twin(L, np.array([-1.0, 40.0, -1.0]), np.array([1.0, 41.0, 1.0]), None, w)[0]
    assert np.all(f == 0.0)                                                                # [40, 41]: 0, never NaN
    one = bc.twin(np.array([[0.7]]), np.array([-0.2]), np.array([0.9]), np.array([0.1]), np.zeros((0, n)))[0]
    assert np.all(one == special.ndtr((0.9 - 0.1) / 0.7) - special.ndtr((-0.2 - 0.1) / 0.7))
    assert bc.tree_mean(one, 0, M=1) == one[0]                                              # M = 1 uses no point


def test_reflection_keeps_the_upper_tail():
    """M = 1, lo = 6: Phi(-6) with the reflection to what exp(-x^2 / 2) allows in fp64 (the rounding of x^2 / 2 = 18 alone moves it
    by 18 ulp; bc.TAIL6_BOUND), without it to 1e-7: 1 - Phi(6) keeps 2^-53 of 1 on a value of 1e-9"""
    import mpmath
    args = (np.array([[1.0]]), np.array([6.0]), np.array([np.inf]), None, np.zeros((0, 1)))
    with mpmath.workdps(40):
        exact = mpmath.ncdf(-6)
        rel = float(abs(bc.twin(*args)[0][0] - exact) / exact)
        rel_plain = float(abs(bc.twin(*args, reflect=False)[0][0] - exact) / exact)
    print("Phi(-6): relative error {:.3g} with the reflection, {:.3g} without".format(rel, rel_plain))
    assert rel <= bc.TAIL6_BOUND < 1e-9 < rel_plain


def test_scenarios_agree_with_the_twin():
    """the fraction of 2^16 Gaussian-copula scenarios (the latent normals of the joint entry) inside a box of probability about 0.2
    against the twin's probability, within 5 binomial standard errors"""
    L = np.linalg.cholesky(jc.CORR3)
    lo, hi = np.array([0.0, -np.inf, -1.0]), np.array([np.inf, 0.9, 0.8])
    n = 2 ** 16
    y = L @ jc.normals(1234, [0, 1, 2], 0, n)
    frac = np.mean(np.all((y > lo[:, None]) & (y < hi[:, None]), axis=0))
    reps = [bc.tree_mean(bc.twin(L, lo, hi, None, bc.points(s, [0, 1], 0, bc.CLOSED_N, True))[0], 0) for s in bc.SEEDS8]
    prob, stderr = bc.summary(reps)
    print("box {:.6f} +- {:.2g}, scenarios {:.6f}".format(prob, stderr, frac))
    assert 0.1 < prob < 0.3 and abs(frac - prob) <= 5 * np.sqrt(prob * (1 - prob) / n) + 5 * stderr


# ---- argument errors: raised before anything touches the device ---------------------------------------------------------------
def _sd():
    from mlmc_amd.tool import simple_distribution
    return simple_distribution


EYE2 = np.eye(2)


@pytest.mark.parametrize("kw,match", [
    (dict(factor=np.ones((2, 3))), "square"),
    (dict(factor=np.ones(3)), "square"),
    (dict(factor=np.eye(bc.MAX_M + 1), lower=-1.0, upper=1.0), "cap"),
    (dict(factor=np.diag([1.0, 0.0])), "row 1"),
    (dict(factor=np.diag([-1.0, 1.0])), "row 0"),
    (dict(factor=np.diag([1.0, np.inf])), "row 1"),
    (dict(factor=np.array([[1.0, 0.0], [np.nan, 1.0]])), "row 1"),
    (dict(lower=[0.0, 0.0, 0.0]), "broadcast"),
    (dict(lower=np.zeros((2, 2, 2))), "broadcast"),
    (dict(lower=np.zeros((3, 2)), upper=np.ones((4, 2))), "broadcast"),
    (dict(lower=[[0.0, 0.0], [0.0, np.nan]]), "box 1, component 1"),
    (dict(upper=[np.nan, 1.0]), "box 0, component 0"),
    (dict(shift=np.zeros((3, 2))), "shift"),
    (dict(shift=[0.0, np.inf]), "shift"),
    (dict(n=0), "n must"),
    (dict(n=2.5), "n must"),
    (dict(n=True), "n must"),
    (dict(first=-1), "first"),
    (dict(first=2 ** 52), "2\\^52"),
    (dict(seeds=[]), "seed"),
    (dict(seeds=5), "seeds"),
    (dict(seeds=[-1]), "seeds"),
    (dict(seeds=[2 ** 64]), "seeds"),
    (dict(seeds=[1.5]), "seeds"),
    (dict(streams=[0, 1]), "streams"),
    (dict(streams=[-1]), "streams"),
    (dict(streams=[1024]), "1024"),
    (dict(streams=[0.5]), "streams"),
])
def test_copula_box_probabilities_argument_errors(kw, match):
    args = dict(factor=EYE2, lower=[-1.0, -1.0], upper=[1.0, 1.0], n=64, seeds=[0, 1])
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        _sd().copula_box_probabilities(**args)


def _fake(domain=(0.0, 1.0), n_intervals=64, degree=21):
    return types.SimpleNamespace(domain=domain, n_intervals=n_intervals, _gauss_degree=degree)


@pytest.mark.parametrize("kw,match", [
    (dict(distrs=[]), "no distributions"),
    (dict(corr=None), "exactly one"),
    (dict(factor=EYE2), "exactly one"),
    (dict(corr=np.eye(3)), "corr must be"),
    (dict(corr=None, factor=np.ones((3, 1))), "factor"),
    (dict(corr=None, factor=np.array([[1.0, np.nan], [0.0, 1.0]])), "factor"),
    (dict(distrs=[_fake(), _fake(n_intervals=32)]), "same quadrature"),
    (dict(n=0), "n must"),
    (dict(seeds=[]), "seed"),
    (dict(first=-3), "first"),
    (dict(lower=[0.1, 0.2, 0.3]), "broadcast"),
    (dict(lower=[np.nan, 0.2]), "NaN"),
    (dict(given=[0]), "given"),
    (dict(given={2: 0.5}), "component 2"),
    (dict(given={0: 0.5, 1: 0.5}), "nothing is left"),
    (dict(given={0: 0.5}), "broadcast"),                                       # the boxes range over the one free component
    (dict(given={0: [0.5, 0.6]}, lower=np.zeros((3, 1)), upper=np.ones((3, 1))), "2 sets"),
    (dict(streams=[0, 1]), "streams"),
    (dict(lower=-np.inf, upper=np.inf, streams=[0]), "streams"),                # nothing is constrained: no coordinate
])
def test_joint_probabilities_argument_errors(kw, match):
    args = dict(distrs=[_fake(), _fake()], lower=[0.2, 0.2], upper=[0.8, 0.8], n=64, seeds=[0, 1], corr=EYE2)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        _sd().joint_probabilities(**args)


def test_joint_probabilities_without_a_constraint_needs_no_device():
    """limits at or beyond the ends of the domains are infinite scores: every component drops and the probability is 1"""
    res = _sd().joint_probabilities([_fake(), _fake((-2.0, 3.0))], [[0.0, -2.0], [-np.inf, -5.0]], [1.0, np.inf], 64, [0, 1, 2], corr=EYE2)
    assert np.array_equal(res.prob, [1.0, 1.0]) and np.array_equal(res.stderr, [0.0, 0.0]) and res.replicates.shape == (3, 2)
    assert res.n == 64 and np.array_equal(res.seeds, [0, 1, 2])
    one = _sd().joint_probabilities([_fake()], -np.inf, np.inf, 8, [4], corr=np.eye(1), return_integrand=True)
    assert one[1] is None and np.isnan(one[0].stderr[0]) and one[0].prob[0] == 1.0


@pytest.mark.parametrize("call,kw,match", [
    ("estimate_joint_probability", dict(n=0), "n must"),
    ("estimate_joint_probability", dict(seeds=()), "seed"),
    ("estimate_joint_probability", dict(seeds=[0.5]), "seeds"),
    ("estimate_joint_probability", dict(first=-1), "first"),
    ("estimate_joint_probability", dict(lower=[np.nan, 0.0]), "NaN"),
    ("estimate_joint_probability", dict(corr="pearson"), "corr must be"),
    ("estimate_joint_exceedance", dict(thresholds=[np.nan, 0.0]), "NaN"),
    ("estimate_joint_exceedance", dict(n=-4), "n must"),
    ("estimate_joint_exceedance", dict(corr="x"), "corr must be"),
])
def test_estimate_argument_errors(call, kw, match):
    from mlmc_amd.estimator import Estimate
    est = Estimate(None, None, None)
    args = dict(lower=[0.0, 0.0], upper=[1.0, 1.0]) if call == "estimate_joint_probability" else dict(thresholds=[0.0, 0.0])
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        getattr(est, call)(**args)
