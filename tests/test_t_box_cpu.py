"""CPU tests of the Student-t box probabilities and event scenarios: the host map of limits to t scores against mpmath, its symmetry
and infinities, the argument checks of every changed Python entry (all raised before anything touches the device), and the NumPy twin
of the t chain against SciPy's multivariate t.  Nothing here touches a device."""
import numpy as np
import pytest
from scipy import special, stats

from mlmc_amd import estimator
from mlmc_amd.tool import simple_distribution as sd
from tests import box_prob_cases as bc
from tests import t_box_cases as tb


def test_limit_mapping_against_mpmath():
    zn = special.ndtri(tb.LEVELS)
    worst = 0.0
    for dof in tb.DOFS:
        y = sd.t_scores(zn, dof)
        ulps = np.array([tb.score_ulps(a, tb.mp_t_score(dof, z)) for a, z in zip(y, zn)])
        i = int(np.argmax(ulps))
        print("t_scores, nu = {:g}: at most {:.3g} ulps of the score (level {:g}), median {:.2f}".format(
            dof, ulps[i], tb.LEVELS[i], float(np.median(ulps))))
        worst = max(worst, float(ulps[i]))
    print("largest: {:.4g} ulps; recorded {:.4g}, gate {:.4g}".format(worst, tb.T_SCORE_ULPS_OBSERVED, tb.T_SCORE_ULPS_GATE))
    assert worst <= tb.T_SCORE_ULPS_GATE


def test_mapping_symmetry_and_infinities():
    z = np.concatenate([special.ndtri(tb.LEVELS), [-37.0, 37.0, 8.2, -8.2]])
    for dof in tb.DOFS:
        y = sd.t_scores(z, dof)
        assert np.array_equal(sd.t_scores(-z, dof), -y)                                    # odd, bit for bit
        finite = y[np.isfinite(y)]
        assert np.all(np.diff(finite[np.argsort(z[np.isfinite(y)])]) >= 0)                  # monotone
        assert np.all(np.abs(y[z != 0]) >= np.abs(z[z != 0]) * (1 - 1e-9))                   # heavier tails: |y| >= |z|
    edge = sd.t_scores(np.array([[-np.inf, np.inf], [0.0, np.nan]]), 3)
    assert edge.shape == (2, 2) and edge[0, 0] == -np.inf and edge[0, 1] == np.inf and edge[1, 0] == 0.0 and np.isnan(edge[1, 1])
    # the map is the quantile transform between the two laws
    assert abs(stats.t.cdf(sd.t_scores(-1.3, 7.5), 7.5) - special.ndtr(-1.3)) < 1e-12


def _box(fn, **kw):
    eye, lo, hi = np.eye(3), [-1.0] * 3, [1.0] * 3
    return fn(eye, lo, hi, 64, [0], **kw)


@pytest.mark.parametrize("fn", [sd.copula_box_probabilities, sd.copula_box_draws], ids=["probabilities", "draws"])
def test_argument_errors_of_the_score_entries(fn):
    for bad in (0.5, 65.0, np.nan, True, "three"):
        with pytest.raises(ValueError, match="dof must lie in"):
            _box(fn, dof=bad)
    with pytest.raises(ValueError, match="dof together with shift"):
        _box(fn, dof=3, shift=np.zeros(3))
    with pytest.raises(ValueError, match="need dof"):
        _box(fn, mix_stream=5)
    with pytest.raises(ValueError, match="need dof"):
        _box(fn, return_mixing=True)
    with pytest.raises(ValueError, match="need dof"):
        _box(fn, dof=np.inf, mix_stream=5)
    count = 2 if fn is sd.copula_box_probabilities else 3
    with pytest.raises(ValueError, match="mix_stream must be given"):
        _box(fn, dof=3, streams=list(range(4, 4 + count)))
    with pytest.raises(ValueError, match="mix_stream 5 is the stream of"):
        _box(fn, dof=3, streams=list(range(4, 4 + count)), mix_stream=5)
    with pytest.raises(ValueError, match="mix_stream 2 is the stream of"):                  # the default chain streams are 1 .. count
        _box(fn, dof=3, mix_stream=2)
    with pytest.raises(ValueError, match="mix_stream must be an integer"):
        _box(fn, dof=3, mix_stream=-1)
    with pytest.raises(ValueError, match="below 1024"):
        _box(fn, dof=3, mix_stream=1024)
    with pytest.raises(ValueError, match="below 1024"):
        _box(fn, dof=3, streams=list(range(1023, 1023 + count)), mix_stream=0)


def test_argument_errors_of_the_entries_in_own_units():
    two = [object()] * 2
    for fn, name in ((sd.joint_probabilities, "joint_probabilities"), (sd.event_samples, "event_samples")):
        with pytest.raises(ValueError, match="^" + name + ": dof together with given"):
            fn(two, -np.inf, 0.0, 64, [0], corr=np.eye(2), dof=3, given={0: 0.1})
        with pytest.raises(ValueError, match="dof must lie in"):
            fn(two, -np.inf, 0.0, 64, [0], corr=np.eye(2), dof=0.99)
        with pytest.raises(ValueError, match="mix_stream needs dof"):
            fn(two, -np.inf, 0.0, 64, [0], corr=np.eye(2), mix_stream=0)
    with pytest.raises(ValueError, match="dof together with given"):
        sd.joint_aggregates(two, 4, 1, corr=np.eye(2), dof=3, given={0: 0.1})


class _NoWalk(estimator.Estimate):
    """an Estimate whose quantity must not be touched: the checks under test come first"""

    def __init__(self):
        pass


def test_estimate_argument_errors():
    est = _NoWalk()
    calls = (("estimate_joint_probability", lambda **kw: est.estimate_joint_probability(-np.inf, 0.0, corr=np.eye(2), **kw)),
             ("estimate_joint_exceedance", lambda **kw: est.estimate_joint_exceedance(0.0, corr=np.eye(2), **kw)),
             ("sample_given_event", lambda **kw: est.sample_given_event(64, -np.inf, 0.0, corr=np.eye(2), **kw)),
             ("estimate_event_means", lambda **kw: est.estimate_event_means(-np.inf, 0.0, corr=np.eye(2), **kw)))
    for name, call in calls:
        for bad in (0.5, 100.0, np.nan):
            with pytest.raises(ValueError, match="dof must lie in"):
                call(dof=bad)
        with pytest.raises(ValueError, match="dof together with given"):
            call(dof=3, given={0: 0.1})
    for call in (lambda **kw: est.bootstrap_joint_probability(-np.inf, 0.0, n_subsamples=4, seed=1, **kw),
                 lambda **kw: est.bootstrap_joint_exceedance(0.0, n_subsamples=4, seed=1, **kw)):
        with pytest.raises(ValueError, match="dof must lie in"):
            call(dof=0.5)


# ---- the identity P(l < Y < h) = E_s[P(l / s < F z < h / s)] on the twin --------------------------------------------------------------
TWIN_DOF = 3.0
TWIN_LO, TWIN_HI = np.array([-0.5, -np.inf, -1.0]), np.array([np.inf, 0.5, 0.6])
TWIN_N = 2 ** 14


def _twin_inputs(seed, n):
    s = np.sqrt(TWIN_DOF / stats.chi2.ppf(tb.mixing_points(seed, 0, n, False), TWIN_DOF))
    return s, bc.points(seed, tb.chain_streams(3), 0, n, False)


def test_twin_is_the_gaussian_twin_on_the_scaled_limits():
    """t_twin is vectorised over the points; point by point it is tests/box_prob_cases.twin called with lo / s, hi / s, bit for bit"""
    L = np.linalg.cholesky(bc.CORR3)
    s, w = _twin_inputs(5, 24)
    lo, hi = np.array([-0.5, -np.inf, 0.7]), np.array([np.inf, 0.5, 0.6])                   # the last component is empty at every point
    for box in ((TWIN_LO, TWIN_HI), (lo, hi)):
        f = tb.t_twin(L, box[0], box[1], s, w)
        for j in range(s.size):
            want, _ = bc.twin(L, box[0] / s[j], box[1] / s[j], None, w[:, j:j + 1])
            assert np.array_equal(f[j:j + 1].view(np.uint64), want.view(np.uint64))
    assert np.all(tb.t_twin(L, lo, hi, s, w) == 0.0)


def test_twin_against_scipy_multivariate_t():
    """pins the identity, not the kernel: 8 Philox seeds at n = 2^14, s from SciPy's chi-square quantile, against SciPy's own
    multivariate t integral (Genz's lattice rule); the gate is 6 standard errors of the 8 means plus the error SciPy reports"""
    from scipy.stats._qmvnt import _qmvt
    L = np.linalg.cholesky(bc.CORR3)
    means = []
    for seed in bc.SEEDS8:
        s, w = _twin_inputs(seed, TWIN_N)
        means.append(tb.t_twin(L, TWIN_LO, TWIN_HI, s, w).mean())
    prob, stderr = bc.summary(means)
    want, abseps, _ = _qmvt(200000, TWIN_DOF, bc.CORR3, TWIN_LO, TWIN_HI, np.random.default_rng(0))
    public = stats.multivariate_t.cdf(TWIN_HI, np.zeros(3), bc.CORR3, TWIN_DOF, lower_limit=TWIN_LO, maxpts=200000,
                                      random_state=np.random.default_rng(0))
    gauss, _ = bc.summary([bc.twin(L, TWIN_LO, TWIN_HI, None, _twin_inputs(seed, TWIN_N)[1])[0].mean() for seed in bc.SEEDS8])
    print("twin {:.6f} +- {:.2g}, SciPy {:.6f} +- {:.2g} (3 standard errors), the Gaussian box {:.6f}".format(
        prob, stderr, want, abseps, gauss))
    assert float(public) == float(want)
    assert 0.15 < want < 0.25
    assert abs(prob - want) <= 6.0 * stderr + abseps
    assert abs(gauss - want) > 6.0 * stderr + abseps                                       # the mixing is what the test sees
