"""GPU tests of the aggregates of joint scenarios through the Python layer, on a six-component vector quantity:
tool.simple_distribution.scenario_aggregates / joint_aggregates / row_statistics / event_aggregates and Estimate.estimate_aggregates."""
import numpy as np
import pytest

from tests import aggregate_cases as ac

pytestmark = pytest.mark.gpu

M_TIMES, M_ARR = 2, 3          # result format: times [1, 2], one location, array (3, 1) -> M = 6 components
LOG_COMP = 4
M = M_TIMES * M_ARR
SEED = 20240607
U = 2.0 ** -53


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


def _vector_levels():
    """Six components of different distributions; NaNs at different samples of different components, values outside one
    component's own domain only, one strictly positive component (log moments)."""
    from tests.util import level_arrays
    steps = [0.5, 0.07, 0.01]
    levels = level_arrays([20000, 4000, 1200], steps, M, 0, seed=77)
    shift = [0.0, 0.3, -0.4, 0.1, 0.0, -0.2]
    scale = [1.0, 0.7, 1.2, 0.9, 0.25, 1.1]
    out = []
    for l, (f, c) in enumerate(levels):
        f = f.copy()
        c = None if c is None else c.copy()
        for m in range(f.shape[0]):
            for arr in (f,) if c is None else (f, c):
                arr[m] = shift[m] + scale[m] * (arr[m] - 0.125 * m)
                if m == LOG_COMP:
                    arr[m] = np.exp(arr[m])
        f[1, 7::53] = np.nan
        f[3, 11::41] = np.nan
        if c is not None:
            c[2, 5::37] = np.nan
        f[5, 3::151] = 40.0                    # far outside component 5's own domain
        out.append((f, c))
    return out, steps


def _vector_storage(chunk_size):
    from mlmc_amd.sample_storage import Memory
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    levels, steps = _vector_levels()
    spec = [QuantitySpec(name="q", unit="m", shape=(M_ARR, 1), times=[1, 2], locations=['0'])]
    st = Memory(chunk_size=chunk_size)
    st.save_global_data(result_format=spec, level_parameters=[[s] for s in steps])
    for l, (f, c) in enumerate(levels):
        st.set_level_samples(l, f.T, None if c is None else c.T)
    st.save_n_ops([(l, (float(len(levels[l][0][0])), len(levels[l][0][0]))) for l in range(len(levels))])
    return st, spec


@pytest.fixture(scope="module")
def fitted(hip):
    """(Estimate, densities, distributions, corr [6, 6], the marginal 0.2 / 0.5 / 0.9 quantiles [3, 6])"""
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.tool import simple_distribution as sd
    st, spec = _vector_storage(None)
    root = make_root_quantity(st, spec)['q']
    comps = [root[t]['0'][i, 0] for t in (1, 2) for i in range(M_ARR)]
    fns = [Legendre(9 + 2 * m, Estimate.estimate_domain(q_m, st), log=(m == LOG_COMP)) for m, q_m in enumerate(comps)]
    est = Estimate(root, st, fns[0])
    pdfs = est.construct_densities(tol=1e-8, orth_moments_tol=1e-4, moments_fns=fns)
    distrs = [d[0] for d in pdfs]
    assert all(bool(d[2].success) for d in pdfs)
    corr = np.full((M, M), 0.5)
    np.fill_diagonal(corr, 1.0)
    marg = np.stack([sd.quantiles([d], [np.array([0.2, 0.5, 0.9])])[0] for d in distrs], axis=1)
    return est, pdfs, distrs, corr, marg


def _host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else a


def _agg_args(marg):
    w = np.array([[1.0, 1.0, 1.0, 1.0, 1.0, 1.0], [0.5, -2.0, 0.25, 3.0, 0.0, 1.5]])
    return dict(weights=w, lower=marg[0], upper=marg[2], members=[1, 1, 0, 1, 1, 1], extremes=("max", "min", "argmax", "argmin"))


@pytest.mark.parametrize("qmc", [False, True])
def test_joint_aggregates_do_not_depend_on_the_block(hip, fitted, qmc):
    """joint_aggregates in blocks of 64, 1000 and n columns = scenario_aggregates of the whole scenario matrix, bit for bit"""
    from mlmc_amd.tool import simple_distribution as sd
    _, _, distrs, corr, marg = fitted
    n = 4096 + 37
    kw = _agg_args(marg)
    x = sd.joint_samples(distrs, n, SEED, corr=corr, qmc=qmc)
    want = sd.scenario_aggregates(x, **kw)
    assert want.names == ["linear0", "linear1", "max", "min", "count", "argmax", "argmin"] and want.rows.shape == (7, n)
    assert ac.same_bits(want.rows, ac.aggregates_reference(x[None], kw["weights"], np.array(kw["members"]), kw["lower"], kw["upper"], 31)[0])
    for block in (64, 1000, n):
        got = sd.joint_aggregates(distrs, n, SEED, corr=corr, qmc=qmc, block=block, **kw)
        assert got.names == want.names and ac.same_bits(got.rows, want.rows), block
    dev = sd.joint_aggregates(distrs, n, SEED, corr=corr, qmc=qmc, block=1000, device=True, **kw)
    assert dev.rows.is_cuda and ac.same_bits(_host(dev.rows), want.rows)
    # a window of the draw indices: first = 50, n = 100 are the columns [50, 150)
    part = sd.joint_aggregates(distrs, 100, SEED, corr=corr, qmc=qmc, block=64, first=50, **kw)
    assert ac.same_bits(part.rows, want.rows[:, 50:150])
    # device draws are read in place and give the bits of the host draws
    xd = sd.joint_samples(distrs, n, SEED, corr=corr, qmc=qmc, device=True)
    assert ac.same_bits(_host(sd.scenario_aggregates(xd, **kw).rows), want.rows)


def test_joint_aggregates_given(hip, fitted):
    """with given = {0: [v1, v2, v3]}: the aggregates of conditional_samples, a leading axis of three sets, for every block"""
    from mlmc_amd.tool import simple_distribution as sd
    _, _, distrs, corr, marg = fitted
    n = 4096 + 37
    kw = _agg_args(marg)
    given = {0: marg[:, 0].copy()}
    x = sd.conditional_samples(distrs, n, SEED, given, corr=corr)
    assert x.shape == (3, M, n)
    want = sd.scenario_aggregates(x, **kw)
    assert want.rows.shape == (3, 7, n)
    assert ac.same_bits(want.rows, ac.aggregates_reference(x, kw["weights"], np.array(kw["members"]), kw["lower"], kw["upper"], 31))
    for block in (64, 1000, n):
        got = sd.joint_aggregates(distrs, n, SEED, corr=corr, given=given, block=block, **kw)
        assert ac.same_bits(got.rows, want.rows), block
    one = sd.joint_aggregates(distrs, n, SEED, corr=corr, given={0: float(marg[1, 0])}, block=1000, **kw)
    assert one.rows.shape == (7, n) and ac.same_bits(one.rows, want.rows[1])


def test_comonotone_total(hip, fitted):
    """factor = ones [M, 1] and positive weights: every component is a non-decreasing function of ONE normal, so the order statistics of
    the total are the weighted sums of the components' order statistics and every np.percentile of the total equals
    sum_m w_m * the same np.percentile of row m up to rounding.  The chain takes M rounded products and M rounded sums, each within one
    unit 2^-53 of sum |w_m x_m|: the bound is M such units (the interpolation of np.percentile is linear and adds no term of its
    own beyond them at this size)."""
    from mlmc_amd import engine
    from mlmc_amd.tool import simple_distribution as sd
    _, _, distrs, _, _ = fitted
    n = 4096
    w = np.array([1.0, 0.5, 2.0, 0.75, 3.0, 1.25])
    x = sd.joint_samples(distrs, n, SEED, factor=np.ones((M, 1)), device=True)
    total = sd.scenario_aggregates(x, weights=w).rows
    probs = np.array([0.0, 1.0, 5.0, 25.0, 50.0, 75.0, 95.0, 99.0, 100.0])
    q_total = engine.row_percentiles(total, probs)[0]
    q_rows = engine.row_percentiles(x, probs)
    xh = _host(x)
    assert ac.same_bits(q_total, np.percentile(_host(total)[0], probs)) and ac.same_bits(q_rows[2], np.percentile(xh[2], probs))
    want = (w[:, None] * q_rows).sum(axis=0)
    bound = M * U * (np.abs(w[:, None] * q_rows)).sum(axis=0)
    print("comonotone total: worst distance {:.3f} of the bound".format(np.max(np.abs(q_total - want) / bound)))
    assert np.all(np.abs(q_total - want) <= bound)


def test_count_row_is_the_box_event(hip, fitted):
    """count == 0 is the NumPy box test on the same draws; as a sanity check, P(N = 0) of estimate_aggregates lies within 6 combined
    standard errors of estimate_joint_probability for a box of probability about 0.3 (limits at the marginal 0.2 and 0.9 quantiles of
    four components)"""
    from mlmc_amd.tool import simple_distribution as sd
    est, pdfs, distrs, corr, marg = fitted
    lower, upper = marg[0].copy(), marg[2].copy()
    lower[4:], upper[4:] = -np.inf, np.inf
    x = sd.joint_samples(distrs, 4096, SEED, corr=corr)
    agg = sd.scenario_aggregates(x, lower=lower, upper=upper)
    assert agg.names == ["count"]
    box = np.all((lower[:, None] < x) & (x < upper[:, None]), axis=0)
    assert np.array_equal(agg.rows[0] == 0, box) and agg.rows[0].max() <= 4
    res, ok = est.estimate_aggregates(lower=lower, upper=upper, extremes=(), n=4096, seeds=tuple(range(8)), corr=corr, densities=pdfs)
    ref, _ = est.estimate_joint_probability(lower, upper, n=4096, seeds=tuple(range(8)), corr=corr, densities=pdfs)
    assert ok.all() and res.names == ["count"] and res.count_prob.shape == (M + 1,)
    assert abs(res.count_prob.sum() - 1.0) <= 1e-12 and np.all(res.count_prob[5:] == 0.0)
    print("P(N = 0) = {:.5f} +- {:.5f}, box probability {:.5f} +- {:.5f}".format(res.count_prob[0], res.count_prob_stderr[0],
                                                                               ref.prob[0], ref.stderr[0]))
    assert 0.15 < ref.prob[0] < 0.5
    assert abs(res.count_prob[0] - ref.prob[0]) <= 6 * np.hypot(res.count_prob_stderr[0], ref.stderr[0])


def test_row_statistics_against_numpy(hip, fitted):
    from mlmc_amd.tool import simple_distribution as sd
    _, _, distrs, corr, marg = fitted
    rows = sd.joint_aggregates(distrs, 5000, SEED, corr=corr, block=2048, device=True, **_agg_args(marg)).rows
    y = _host(rows)
    f = np.random.default_rng(3).uniform(0.0, 1.0, 5000)
    f[::7] = 0.0
    t = np.quantile(y, [0.1, 0.9], axis=1).T
    for weights in (None, f):
        fv = np.ones(5000) if weights is None else weights
        for tail in ("upper", "lower"):
            st = sd.row_statistics(rows, f=weights, thresholds=t, tail=tail)
            host = sd.row_statistics(y, f=weights, thresholds=t, tail=tail)
            for a, b in zip(st, host):
                assert np.array_equal(a, b, equal_nan=True)
            mean = (fv * y).sum(axis=1) / fv.sum()
            var = (fv * (y - mean[:, None]) ** 2).sum(axis=1) / fv.sum()
            ind = (y >= t[:, :1]) if tail == "upper" else (y <= t[:, :1])
            assert np.allclose(st.mean, mean, rtol=1e-12, atol=0) and np.allclose(st.var, var, rtol=1e-11, atol=0)
            assert np.allclose(st.tail_prob[:, 0], (fv * ind).sum(axis=1) / fv.sum(), rtol=1e-12)
            assert np.allclose(st.tail_mean[:, 0], (fv * ind * y).sum(axis=1) / (fv * ind).sum(axis=1), rtol=1e-12)
            assert np.array_equal(st.n_used, np.full(7, 5000)) and np.allclose(st.weight_sum, fv.sum(), rtol=1e-13)
    one = sd.row_statistics(rows[0], thresholds=t[0])
    assert one.mean.shape == () and one.tail_prob.shape == (2,) and one.mean == sd.row_statistics(rows).mean[0]


def test_event_statistics(hip, fitted):
    """with event = (t, inf) the weighted mean of a unit-weight aggregate is estimate_event_means of that component, within the
    rounding of two different summation orders: relative 1e-12, the package's habitual gate for reordered fp64 sums of this size"""
    from mlmc_amd.tool import simple_distribution as sd
    est, pdfs, distrs, corr, marg = fitted
    t = np.array([-np.inf, marg[2, 1], -np.inf, marg[1, 3], -np.inf, -np.inf])
    kw = dict(n=1024, seeds=(0, 1, 2, 3), corr=corr, densities=pdfs)
    res, ok = est.estimate_aggregates(weights=np.eye(M), event=(t, np.inf), extremes=("max",), **kw)
    ref, _ = est.estimate_event_means(t, np.inf, **kw)
    assert res.names == ["linear{}".format(m) for m in range(M)] + ["max", "argmax"]
    assert res.mean.shape == (1, M + 2) and res.quantiles.shape == (1, M + 2, 3) and res.worst_prob.shape == (1, M)
    rel = np.abs(res.mean[0, :M] - ref.mean[0]) / np.abs(ref.mean[0])
    print("event means: worst relative distance {:.3e}".format(rel.max()))
    assert np.all(rel <= 1e-12)
    assert np.allclose(res.mean_stderr[0, :M], ref.stderr[0], rtol=1e-9)
    assert ac.same_bits(res.prob.replicates, ref.prob.replicates)
    assert res.mean[0, 1] > marg[2, 1] and np.all(res.quantiles[0, 1] > marg[2, 1]) and abs(res.worst_prob.sum() - 1.0) <= 1e-12
    assert res.count_prob is None and res.best_prob is None
    # event_aggregates on host scenarios gives the bits of the device path
    scen = sd.event_samples(distrs, t, np.inf, 256, (5, 6), corr=corr)
    ev = sd.event_aggregates(scen, weights=np.eye(M)[:2], extremes=("max", "argmax"))
    assert ev.rows.shape == (2, 1, 4, 256) and ev.weights is scen.weights
    assert ac.same_bits(ev.rows, ac.aggregates_reference(scen.draws.reshape(2, M, 256), np.eye(M)[:2], None, None, None, 9).reshape(2, 1, 4, 256))


def test_aggregate_summary_shapes(hip, fitted):
    """one seed: every stderr is NaN (as in JointProbability); given arrays give a leading axis; a row that is absent gives None"""
    est, pdfs, distrs, corr, marg = fitted
    w = np.ones((2, M))
    res, ok = est.estimate_aggregates(weights=w, probs=(0.1, 0.9), n=2048, seeds=(3,), corr=corr, lower=marg[0], upper=marg[2],
                                      densities=pdfs)
    Q = 7
    assert ok.shape == (M,) and res.names == ["linear0", "linear1", "max", "min", "count", "argmax", "argmin"]
    assert res.quantiles.shape == (Q, 2) and res.shortfall.shape == (Q, 2) and res.mean.shape == (Q,) and res.var.shape == (Q,)
    assert res.count_prob.shape == (M + 1,) and res.worst_prob.shape == (M,) and res.best_prob.shape == (M,)
    for v in (res.quantiles_stderr, res.mean_stderr, res.var_stderr, res.shortfall_stderr, res.count_prob_stderr, res.worst_prob_stderr,
              res.best_prob_stderr):
        assert np.all(np.isnan(v))
    assert res.prob is None and res.n == 2048 and list(res.seeds) == [3] and np.array_equal(res.probs, [0.1, 0.9])
    assert ac.same_bits(res.quantiles[0], res.quantiles[1]) and np.all(res.shortfall[0] >= res.quantiles[0])
    assert abs(res.count_prob.sum() - 1) <= 1e-12 and abs(res.worst_prob.sum() - 1) <= 1e-12 and abs(res.best_prob.sum() - 1) <= 1e-12
    low, _ = est.estimate_aggregates(weights=w, probs=(0.1, 0.9), n=2048, seeds=(3,), corr=corr, densities=pdfs, tail="lower", qmc=False)
    assert low.count_prob is None and np.all(low.shortfall[0] <= low.quantiles[0]) and low.names[-1] == "argmin"
    fan, _ = est.estimate_aggregates(weights=w, n=1024, seeds=(0, 1), corr=corr, given={0: marg[:, 0].copy()}, extremes=(), densities=pdfs)
    assert fan.names == ["linear0", "linear1"] and fan.quantiles.shape == (3, 2, 3) and fan.mean.shape == (3, 2)
    assert fan.worst_prob is None and np.all(np.isfinite(fan.mean_stderr)) and np.all(np.diff(fan.mean[:, 0]) > 0)
