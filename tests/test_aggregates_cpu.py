"""CPU tests of the scenario aggregates: the references the device tests compare against are checked here against exact rational
arithmetic, the fp64 twin of the kernel's summation order fixes the gate of the device sums, and the argument checks of the Python
layer run before any device call (this machine may have no device at all)."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import aggregate_cases as ac


def test_reference_linear_rows_are_the_exact_chains():
    """acc = fl(acc + fl(w * x)) step by step in rationals, on the special columns (NaN, +-inf, 0 * inf, +-0) and some plain ones"""
    S, M, n = 2, 5, 40
    x = ac.scenario_inputs(S, M, n, seed=3)
    W = ac.scenario_weights(3, M, seed=4)
    ref = ac.aggregates_reference(x, W, None, None, None, 0)
    assert ref.shape == (S, 3, n)
    cols = sorted({(7 * k + 3) % n for k in range(9)} | {0, 1, n - 1})
    for s in range(S):
        for a in range(3):
            for j in cols:
                assert ac.same_bits(ref[s, a, j], ac.chain_exact(W[a], x[s, :, j])) or \
                    (np.isnan(ref[s, a, j]) and np.isnan(ac.chain_exact(W[a], x[s, :, j]))), (s, a, j)
    j_inf = (7 * 8 + 3) % n                                                 # +inf under the zero weight of row 0: 0 * inf = NaN
    assert W[0, M // 2] == 0.0 and np.isnan(ref[:, 0, j_inf]).all() and np.isinf(ref[:, 1, j_inf]).all()
    # a unit weight reproduces its row under ==; -0.0 comes back as +0.0 (+0 + (-0) = +0), the one difference in bits
    e = np.zeros((1, M))
    e[0, 0] = 1.0
    row = ac.aggregates_reference(x, e, None, None, None, 0)[:, 0, :]
    fin = np.all(np.isfinite(x[:, 1:, :]), axis=1)                          # elsewhere 0 * NaN, 0 * inf of another component: NaN
    assert np.array_equal(row[fin], x[:, 0, :][fin], equal_nan=True) and np.isnan(row[~fin]).all() and fin.sum() > 60
    j0 = (7 * 6 + 3) % n
    assert np.signbit(x[0, 0, j0]) and row[0, j0] == 0.0 and not np.signbit(row[0, j0])
    assert ac.chain_exact([1.0, 0.0], [-0.0, 5.0]) == 0.0 and not np.signbit(ac.chain_exact([1.0, 0.0], [-0.0, 5.0]))


def test_reference_extremes_and_count_by_hand():
    nan, inf = np.nan, np.inf
    #              j: 0     1     2     3     4
    x = np.array([[[1.0, nan, -0.0, 2.0, -inf],
                   [3.0, 5.0, 0.0, 2.0, nan],
                   [3.0, nan, -0.0, 1.0, 7.0]]])
    every = ac.AGG_MAX | ac.AGG_MIN | ac.AGG_COUNT | ac.AGG_ARGMAX | ac.AGG_ARGMIN
    lo, hi = np.array([0.0, -inf, -inf]), np.array([2.5, 4.0, inf])
    r = ac.aggregates_reference(x, None, None, lo, hi, every)[0]
    vmax, vmin, count, amax, amin = r
    assert amax.tolist() == [1, 0, 0, 0, 1] and amin.tolist() == [0, 0, 0, 2, 1]       # first NaN; first of equal extremes
    assert vmax[0] == 3.0 and np.isnan(vmax[1]) and np.signbit(vmax[2]) and vmax[3] == 2.0 and np.isnan(vmax[4])
    assert vmin[0] == 1.0 and np.isnan(vmin[1]) and np.signbit(vmin[2]) and vmin[3] == 1.0 and np.isnan(vmin[4])
    # component 2 has no finite limit and never counts; a NaN draw of a constrained component counts; 0 < -0.0 is false
    assert count.tolist() == [0, 2, 1, 0, 2]
    mem = np.array([0, 1, 1], dtype=np.uint8)                                          # the NaNs of component 0 are not seen
    r = ac.aggregates_reference(x, None, mem, None, None, ac.AGG_ARGMAX | ac.AGG_MAX | ac.AGG_ARGMIN)[0]
    assert r[1].tolist() == [1, 2, 1, 1, 1] and r[2].tolist() == [1, 2, 1, 2, 1]
    assert r[0][2] == 0.0 and not np.signbit(r[0][2]) and np.isnan(r[0][1]) and np.isnan(r[0][4])
    # count == 0 is the box event
    z = np.random.default_rng(5).standard_normal((1, 3, 500))
    c = ac.aggregates_reference(z, None, None, lo, hi, ac.AGG_COUNT)[0, 0]
    box = np.all((lo[:, None] < z[0]) & (z[0] < hi[:, None]), axis=0)
    assert np.array_equal(c == 0, box) and 0 < box.sum() < 500


@pytest.mark.parametrize("data", ["offset", "lognormal"])
def test_long_double_sums_against_rationals(data):
    """the long-double reference lies within 1/8 of the fp64 unit of the exact sums (it is the yardstick of twin and device)"""
    n = 300
    y, f = ac.sum_row(data, n, 11), ac.sum_weights("zeros", n, 11)
    y[17] = np.nan
    f[40] = np.nan
    assert np.sum(f == 0.0) > 50
    t = ac.row_thresholds(y)
    for c in (0.0, float(np.nansum(f * y) / np.nansum(f))):
        for lower in (False, True):
            used, ld = ac.weighted_sums_ld(y, f, c, t, lower)
            exact = ac.weighted_sums_exact(y, f, c, t, lower)
            assert used == n - 2
            sf, sfd, sfd2 = ac.sum_units(y, f, c)
            for k, (a, b) in enumerate(zip(ld, exact)):
                unit = sfd2 if k == 2 else (sf if k == 0 or (k >= 3 and k % 2 == 1) else sfd)
                assert abs(_fraction_of(a) - b) <= Fraction(unit) / 2 ** 56, (c, lower, k)


def _fraction_of(v):
    """a long double as an exact rational (through its high and low double parts)"""
    hi = float(v)
    lo = float(v - np.longdouble(hi))
    return Fraction(hi) + Fraction(lo)


def test_twin_counts_and_thresholds():
    """with unit weights the tail 'sums' are counts: the >= / <= edge at a data value is exact"""
    y = ac.sum_row("lognormal", 4097, 2)
    y[5::97] = np.nan
    t = ac.row_thresholds(y)
    for lower in (False, True):
        used, s = ac.weighted_sums_twin(y, None, 0.0, t, lower)
        assert used == np.sum(~np.isnan(y)) and s[0] == used
        for k, tk in enumerate(t):
            with np.errstate(invalid="ignore"):
                assert s[3 + 2 * k] == np.sum((y <= tk) if lower else (y >= tk)), (lower, k)
    assert np.any(y == t[3])


def test_twin_distance_and_gate():
    """the fp64 twin of the kernel's order against the long-double reference over the cases the device test uses: its worst distance
    is the recorded one, and the gate is 4 x that, rounded up to a power of two"""
    worst_first = worst_second = 0.0
    count = 0
    for name, y, f, c, t in ac.sum_cases():
        used_t, twin = ac.weighted_sums_twin(y, f, c, t)
        used_r, ref = ac.weighted_sums_ld(y, f, c, t)
        assert used_t == used_r, name
        first, second = ac.distances(twin, ref, ac.sum_units(y, f, c))
        worst_first, worst_second = max(worst_first, first), max(worst_second, second)
        count += 1
    print("twin worst over {} cases: first sums {:.3f}, second sums {:.3f} units".format(count, worst_first, worst_second))
    assert count == 2 * 9 * 3 * 2
    assert worst_first <= ac.TWIN_WORST_FIRST and worst_second <= ac.TWIN_WORST_SECOND
    assert worst_first > 0.5 * ac.TWIN_WORST_FIRST and worst_second > 0.5 * ac.TWIN_WORST_SECOND     # the record is not stale
    assert ac.GATE_FIRST == 2.0 ** math.ceil(math.log2(4.0 * ac.TWIN_WORST_FIRST))
    assert ac.GATE_SECOND == 2.0 ** math.ceil(math.log2(4.0 * ac.TWIN_WORST_SECOND))


def test_abi_declares_and_binds_the_entries():
    from mlmc_amd import _lib
    lib = _lib.load()
    for name in ("mlmc_scenario_aggregates", "mlmc_rows_weighted_sums"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert (_lib.AGG_MAX, _lib.AGG_MIN, _lib.AGG_COUNT, _lib.AGG_ARGMAX, _lib.AGG_ARGMIN) == ac.EXTRA_BITS


# ---- argument checks of the Python layer: all raised before anything touches a device ---------------------------------------------
def test_scenario_aggregates_argument_errors():
    from mlmc_amd.tool import simple_distribution as sd
    x = np.zeros((4, 10))
    with pytest.raises(ValueError, match="scenario_aggregates: weights must be"):
        sd.scenario_aggregates(x, weights=np.ones(3))
    with pytest.raises(ValueError, match="scenario_aggregates: weights must be"):
        sd.scenario_aggregates(x, weights=np.ones((2, 2, 4)))
    with pytest.raises(ValueError, match="weight of row 1, component 2 is not finite"):
        w = np.ones((2, 4))
        w[1, 2] = np.inf
        sd.scenario_aggregates(x, weights=w)
    with pytest.raises(ValueError, match="upper limit of component 3 is NaN"):
        sd.scenario_aggregates(x, lower=-1.0, upper=[1.0, 1.0, 1.0, np.nan])
    with pytest.raises(ValueError, match="lower must broadcast"):
        sd.scenario_aggregates(x, lower=[0.0, 1.0])
    with pytest.raises(ValueError, match="extremes must be among"):
        sd.scenario_aggregates(x, extremes=("largest",))
    with pytest.raises(ValueError, match="members must be a mask"):
        sd.scenario_aggregates(x, members=[1, 0], extremes=("max",))
    with pytest.raises(ValueError, match="no component is a member"):
        sd.scenario_aggregates(x, members=[0, 0, 0, 0], extremes=("max",))
    with pytest.raises(ValueError, match="nothing to compute"):
        sd.scenario_aggregates(x)
    with pytest.raises(ValueError, match="scenario_aggregates: the array must have 2 or 3 axes"):
        sd.scenario_aggregates(np.zeros(5), weights=np.ones(5))
    names = sd._aggregate_args("t", 4, np.ones((2, 4)), None, 1.0, None, ("argmin", "max"))[-1]
    assert names == ["linear0", "linear1", "max", "count", "argmin"]


def test_row_statistics_and_joint_aggregates_argument_errors():
    from mlmc_amd.tool import simple_distribution as sd
    with pytest.raises(ValueError, match="row_statistics: tail must be"):
        sd.row_statistics(np.zeros((2, 5)), tail="both")
    with pytest.raises(ValueError, match="row_statistics: the weights must be"):
        sd.row_statistics(np.zeros((2, 5)), f=np.ones(4))
    with pytest.raises(ValueError, match="row_statistics: thresholds must be"):
        sd.row_statistics(np.zeros((2, 5)), thresholds=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="row_statistics: a threshold is NaN"):
        sd.row_statistics(np.zeros((2, 5)), thresholds=[np.nan])
    distrs = [object(), object()]                               # never looked at: every error below comes first
    eye = np.eye(2)
    with pytest.raises(ValueError, match="joint_aggregates: qmc and antithetic"):
        sd.joint_aggregates(distrs, 8, 1, weights=np.ones(2), corr=eye, antithetic=True, qmc=True)
    with pytest.raises(ValueError, match="joint_aggregates: exactly one of corr and factor"):
        sd.joint_aggregates(distrs, 8, 1, weights=np.ones(2))
    with pytest.raises(ValueError, match="joint_aggregates: block must be"):
        sd.joint_aggregates(distrs, 8, 1, weights=np.ones(2), corr=eye, block=0)
    with pytest.raises(ValueError, match="joint_aggregates: with antithetic, block"):
        sd.joint_aggregates(distrs, 8, 1, weights=np.ones(2), corr=eye, antithetic=True, block=3)
    with pytest.raises(ValueError, match="joint_aggregates: weights must be"):
        sd.joint_aggregates(distrs, 8, 1, weights=np.ones(3), corr=eye)
    with pytest.raises(ValueError, match="joint_aggregates: seed"):
        sd.joint_aggregates(distrs, 8, -1, weights=np.ones(2), corr=eye)
    with pytest.raises(ValueError, match="joint_aggregates: no distributions"):
        sd.joint_aggregates([], 8, 1, weights=np.ones(2), corr=eye)


def test_estimate_aggregates_argument_errors():
    """shapes of the weights, NaN limits, probs outside [0, 1], antithetic with qmc: before densities are constructed"""
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    from mlmc_amd.sample_storage import Memory
    spec = [QuantitySpec(name="q", unit="m", shape=(3, 1), times=[1], locations=['0'])]
    st = Memory()
    st.save_global_data(result_format=spec, level_parameters=[[0.5]])
    st.set_level_samples(0, np.random.default_rng(0).standard_normal((50, 3)), None)
    est = Estimate(make_root_quantity(st, spec)['q'], st)
    with pytest.raises(ValueError, match="estimate_aggregates: weights must be"):
        est.estimate_aggregates(weights=np.ones(4))
    with pytest.raises(ValueError, match="estimate_aggregates: the lower limit of component 1 is NaN"):
        est.estimate_aggregates(weights=np.ones(3), lower=[0.0, np.nan, 0.0])
    with pytest.raises(ValueError, match="estimate_aggregates: probs must be probabilities"):
        est.estimate_aggregates(weights=np.ones(3), probs=(0.5, 1.5))
    with pytest.raises(ValueError, match="estimate_aggregates: qmc and antithetic"):
        est.estimate_aggregates(weights=np.ones(3), antithetic=True)
    with pytest.raises(ValueError, match="estimate_aggregates: extremes must be among"):
        est.estimate_aggregates(weights=np.ones(3), extremes=("argmax",))
    with pytest.raises(ValueError, match="estimate_aggregates: tail must be"):
        est.estimate_aggregates(weights=np.ones(3), tail="both")
    with pytest.raises(ValueError, match="estimate_aggregates: a limit of the event is NaN"):
        est.estimate_aggregates(weights=np.ones(3), event=([np.nan, 0, 0], np.inf))
    with pytest.raises(ValueError, match="estimate_aggregates: at least one seed"):
        est.estimate_aggregates(weights=np.ones(3), seeds=())
