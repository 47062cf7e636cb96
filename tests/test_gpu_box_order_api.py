"""GPU tests of order="genz" above the C ABI: `joint_probabilities` on the named cases of
tests/box_order_cases.py under twelve uniform marginals (the Gaussian copula with and without given values, the t copula with plain
and with conditioned mixing) against order="natural" and against the chain twin at n = 2^16, and the one-call bootstrap bands of
Estimate.bootstrap_joint_exceedance against the loop over the replicates' correlation matrices that they replace, bit for bit."""
import functools

import numpy as np
import pytest
from scipy import special

from tests import box_order_cases as oc
from tests import box_prob_cases as bp
from tests import score_cases as sk
from tests.test_gpu_bootstrap_batch import _memory, _root_q
from tests.test_gpu_joint_samples import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
N = 2 ** 12
SEEDS = list(bp.SEEDS8)
DOF = 3.0


def _sd():
    from mlmc_amd.tool import simple_distribution
    return simple_distribution


@pytest.fixture(scope="module")
def uniform12():
    """twelve uniform marginals on (0, 1): a limit with normal score z is Phi(z) in the component's own units"""
    return [sk.closed_distribution(0.0, (0.0, 1.0)) for _ in range(12)]


def _own_units(case):
    return special.ndtr(case.lo), special.ndtr(case.hi)


@functools.lru_cache(maxsize=None)
def _scores(case):
    """the normal scores that `joint_probabilities` itself gives the limits of the case (one device call, as there)"""
    sd = _sd()
    distrs = [sk.closed_distribution(0.0, (0.0, 1.0)) for _ in range(case.M)]
    lo, hi = _own_units(case)
    z_lo, z_hi, keep, finish = sd._limit_scores("test", distrs, lo, hi)
    finish()
    assert keep.size == case.M
    return z_lo, z_hi


@functools.lru_cache(maxsize=None)
def _reference(case):
    """(prob, stderr) of box 0 from the chain twin at n = 2^16 on the twin's order of the scores the device call sees"""
    z_lo, z_hi = _scores(case)
    low = _sd().correlation_factor(case.C)[0]
    t = oc.order_twin(low @ low.T, z_lo[:1], z_hi[:1])
    p = t.perm[0]
    return oc.reference_probability(t.L[0], z_lo[0][p], z_hi[0][p])


def _agree(a, se_a, b, se_b, what):
    z = abs(a - b) / np.hypot(se_a, se_b)
    print("{}: {:.8g} +- {:.2g} against {:.8g} +- {:.2g}: {:.2f} combined standard errors".format(what, a, se_a, b, se_b, z))
    assert z <= 4.0, what


@pytest.mark.parametrize("case", [oc.ASC, oc.AR], ids=repr)
def test_genz_against_natural_and_the_twin(hip, uniform12, case):
    sd = _sd()
    lo, hi = _own_units(case)
    nat = sd.joint_probabilities(uniform12, lo, hi, N, SEEDS, corr=case.C)
    gz, perm = sd.joint_probabilities(uniform12, lo, hi, N, SEEDS, corr=case.C, order="genz", return_order=True)
    ref, ref_se = _reference(case)
    print("\n{}: natural stderr {:.3g}, reordered {:.3g}: {:.0f} x; reference {:.8g} +- {:.2g}".format(
        case, nat.stderr[0], gz.stderr[0], nat.stderr[0] / gz.stderr[0], ref, ref_se))
    _agree(gz.prob[0], gz.stderr[0], nat.prob[0], nat.stderr[0], "reordered against natural")
    _agree(gz.prob[0], gz.stderr[0], ref, ref_se, "reordered against the twin at n = 2^16")
    _agree(nat.prob[0], nat.stderr[0], ref, ref_se, "natural against the twin at n = 2^16")
    assert gz.stderr[0] * 10.0 <= nat.stderr[0]
    assert perm.shape == (1, 12) and perm.dtype == np.int64 and oc.is_permutation(perm, 12)
    if case is oc.ASC:
        assert np.array_equal(perm[0], np.arange(12)[::-1])
    # order="natural" is the call as it has always been, and reports the caller's order
    same, natural_order = sd.joint_probabilities(uniform12, lo, hi, N, SEEDS, corr=case.C, order="natural", return_order=True)
    assert np.array_equal(same.replicates, nat.replicates) and np.array_equal(natural_order, [np.arange(12)])
    # the reordered call IS the per-box chain on what box_order returns
    z_lo, z_hi = _scores(case)
    low = sd.correlation_factor(case.C)[0]
    o = sd.box_order(low @ low.T, z_lo, z_hi)
    direct = sd.copula_box_probabilities(o.factor, o.lower, o.upper, N, SEEDS)
    assert np.array_equal(o.perm, perm) and np.array_equal(direct.replicates, gz.replicates)


def test_genz_leaves_unconstrained_components_out(hip, uniform12):
    sd = _sd()
    lo, hi = _own_units(oc.ASC)
    lo = lo.copy()
    lo[0, [2, 7]] = -np.inf
    gz, perm = sd.joint_probabilities(uniform12, lo, hi, N, SEEDS, corr=oc.ASC.C, order="genz", return_order=True)
    nat = sd.joint_probabilities(uniform12, lo, hi, N, SEEDS, corr=oc.ASC.C)
    keep = [m for m in range(12) if m not in (2, 7)]
    assert perm.shape == (1, 10) and sorted(perm[0].tolist()) == keep and perm[0, 0] == 11        # original indices; the deepest leads
    _agree(gz.prob[0], gz.stderr[0], nat.prob[0], nat.stderr[0], "\nten constrained components of twelve")


@pytest.mark.parametrize("mixing", ["plain", "conditioned"])
def test_genz_under_the_t_copula(hip, uniform12, mixing):
    sd = _sd()
    # two boxes with different leads: `asc` and its mirror image
    lo = np.concatenate([oc.ASC.lo, oc.ASC.lo[:, ::-1]])
    x_lo = special.ndtr(lo)
    kw = dict(corr=oc.ASC.C, dof=DOF, mixing=mixing)
    nat, nat_order = sd.joint_probabilities(uniform12, x_lo, np.inf, N, SEEDS, return_order=True, **kw)
    calls = []
    inner = sd.copula_box_probabilities

    def counted(*a, **k):
        calls.append(np.ndim(a[0]))
        return inner(*a, **k)

    sd.copula_box_probabilities = counted
    try:
        gz, perm = sd.joint_probabilities(uniform12, x_lo, np.inf, N, SEEDS, order="genz", return_order=True, **kw)
    finally:
        sd.copula_box_probabilities = inner
    assert calls == [3]                                # ONE chain call with one factor per box, whatever the leads
    print()
    for b in range(2):
        _agree(gz.prob[b], gz.stderr[b], nat.prob[b], nat.stderr[b], "dof 3, {} mixing, box {}".format(mixing, b))
    assert oc.is_permutation(perm, 12)
    if mixing == "conditioned":
        assert perm[:, 0].tolist() == [11, 0] and nat_order[:, 0].tolist() == [11, 0]      # the lead of each box stays in front
        assert np.array_equal(np.sort(nat_order[:, 1:], axis=1), nat_order[:, 1:])          # natural: the others ascending
    else:
        # the order comes from the NORMAL scores: that of the Gaussian call
        _, gauss_perm = sd.joint_probabilities(uniform12, x_lo, np.inf, N, SEEDS, corr=oc.ASC.C, order="genz", return_order=True)
        assert np.array_equal(perm, gauss_perm)


def test_genz_with_given_values(hip, uniform12):
    sd = _sd()
    given = {0: 0.3, 5: np.array([0.7, 0.2])}
    free = [m for m in range(12) if m not in given]
    lo = np.concatenate([oc.ASC.lo[:, free], oc.ASC.lo[:, free][:, ::-1]])
    x_lo = special.ndtr(lo)
    nat = sd.joint_probabilities(uniform12, x_lo, np.inf, N, SEEDS, corr=oc.ASC.C, given=given)
    gz, perm = sd.joint_probabilities(uniform12, x_lo, np.inf, N, SEEDS, corr=oc.ASC.C, given=given, order="genz", return_order=True)
    cond = sd.conditional_probabilities(uniform12, x_lo, np.inf, given, N, SEEDS, corr=oc.ASC.C, order="genz")
    print()
    for b in range(2):
        _agree(gz.prob[b], gz.stderr[b], nat.prob[b], nat.stderr[b], "given two components, box {}".format(b))
    assert np.array_equal(np.sort(perm, axis=1), [free, free]) and np.array_equal(cond.replicates, gz.replicates)
    with pytest.raises(ValueError, match='order="genz" is out of scope here'):
        sd.conditional_probabilities(uniform12, x_lo, np.inf, given, N, SEEDS, corr=oc.ASC.C, dof=DOF, order="genz")


# ---- the bands of a joint exceedance: one device call -------------------------------------------------------------------------------
BOOT_N = [300, 120]
BOOT_K = [200, 90]
BOOT_SEED = 5


def _boot_levels():
    rng = np.random.default_rng(41)
    mix = np.array([[1.0, 0.0, 0.0], [0.6, 0.8, 0.0], [-0.3, 0.4, 0.86]])
    out = []
    for l, n in enumerate(BOOT_N):
        f = mix @ rng.normal(size=(3, n)) + np.array([[0.5], [-0.2], [1.0]])
        out.append((f, None if l == 0 else f + 0.2 * 0.5 ** l * rng.normal(size=(3, n))))
    return out


@pytest.fixture(scope="module")
def boot(hip):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    st = _memory(_boot_levels(), 3, chunk_size=150)
    est = Estimate(_root_q(st, 3), st, Legendre(5, (-6.0, 6.0)))
    return est, est.construct_densities()


@pytest.mark.parametrize("dof", [None, DOF], ids=["gauss", "t"])
def test_bands_are_one_call_and_the_bits_of_the_loop(boot, dof):
    from mlmc_amd.estimator import quantile_bands
    sd = _sd()
    est, dens = boot
    distrs = [d[0] for d in dens]
    thresholds = np.array([[1.0, 0.5, -np.inf], [1.5, 0.8, 1.8]])
    nb, n, seeds = 20, 2 ** 10, (0, 1, 2)
    calls = []
    inner = sd.copula_box_probabilities

    def counted(*a, **k):
        calls.append(np.shape(a[0]))
        return inner(*a, **k)

    sd.copula_box_probabilities = counted
    try:
        bands = est.bootstrap_joint_exceedance(thresholds, n_subsamples=nb, sample_vector=BOOT_K, seed=BOOT_SEED, n=n, seeds=seeds,
                                               densities=dens, dof=dof, order="natural")
    finally:
        sd.copula_box_probabilities = inner
    # the loop that the one call replaces, written out
    reps = est.est_bootstrap_component_covariance(nb, sample_vector=BOOT_K, seed=BOOT_SEED)
    base = est.estimate_joint_exceedance(thresholds, n=n, seeds=seeds, densities=dens, dof=dof)[0]
    ok = reps.ok.copy()
    replicates = np.full((nb, 2), np.nan)
    for b in range(nb):
        if ok[b]:
            try:
                replicates[b] = sd.joint_probabilities(distrs, thresholds, np.inf, n, list(seeds), corr=reps.corr[b], dof=dof).prob
            except Exception:
                ok[b] = False
    lo, hi = quantile_bands(replicates[:, None, :], ok[:, None], 0.9)
    assert ok.sum() >= nb - 2
    assert calls == [(2 * (int(ok.sum()) + 1), 3, 3)]      # the estimate and the ok replicates, two boxes each, in ONE call
    assert np.array_equal(bands.replicates, replicates, equal_nan=True) and np.array_equal(bands.ok, ok)
    assert np.array_equal(bands.lo, lo[0]) and np.array_equal(bands.hi, hi[0])
    assert np.array_equal(bands.prob, base.prob) and np.array_equal(bands.stderr, base.stderr) and bands.n_ok == int(ok.sum())
    # reordered bands: the same replicates within the integration error of either
    gz = est.bootstrap_joint_exceedance(thresholds, n_subsamples=nb, sample_vector=BOOT_K, seed=BOOT_SEED, n=n, seeds=seeds,
                                        densities=dens, dof=dof, order="genz")
    assert np.array_equal(gz.ok, ok)
    print()
    for b in range(2):
        _agree(gz.prob[b], gz.stderr[b], bands.prob[b], bands.stderr[b], "bands, box {}, reordered against natural".format(b))


def test_estimate_passes_the_order_through(boot):
    est, dens = boot
    t = np.array([1.5, 0.8, 1.8])
    nat = est.estimate_joint_exceedance(t, n=N, densities=dens)[0]
    gz = est.estimate_joint_exceedance(t, n=N, densities=dens, order="genz")[0]
    same = est.estimate_joint_probability(t, np.inf, n=N, densities=dens, order="genz")[0]
    print()
    _agree(gz.prob[0], gz.stderr[0], nat.prob[0], nat.stderr[0], "estimate_joint_exceedance, reordered against natural")
    assert np.array_equal(gz.replicates, same.replicates)
