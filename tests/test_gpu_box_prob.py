"""GPU tests of the joint box probabilities (mlmc_copula_box_prob_batch and the Python entries above it): the integrand per point
against the extended-precision reference of tests/box_prob_cases.py within the tolerance recorded there, the shapes against the
NumPy twin, the mean as the header's tree of the integrand bit for bit, exact cases, independence of batch / position / f_out /
memory kind / launch split, repeatability, closed forms, agreement with counted scenarios, the conditional law and the Estimate
entries."""
import numpy as np
import pytest

from tests import box_prob_cases as bc
from tests import joint_sample_cases as jc
from tests.test_gpu_conditional_samples import marginals  # noqa: F401  (fixture)
from tests.test_gpu_density_samples import _small_vector_storage
from tests.test_gpu_joint_samples import hip, table  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
U = bc.U


def _sd():
    from mlmc_amd.tool import simple_distribution
    return simple_distribution


def _run(case, **kw):
    args = dict(shift=case.shift, streams=case.streams, first=case.first, qmc=case.qmc, return_integrand=True)
    args.update(kw)
    return _sd().copula_box_probabilities(case.L, case.lo, case.hi, case.n, case.seeds, **args)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _tree_means(f, case):
    return np.array([[bc.tree_mean(f[r, b], case.first, case.M) for b in range(case.B)] for r in range(len(case.seeds))])


@pytest.mark.parametrize("case", bc.POINT_CASES, ids=repr)
def test_integrand_against_reference(hip, case):
    res, f = _run(case)
    assert f.shape == (len(case.seeds), case.B, case.n) and res.replicates.shape == f.shape[:2]
    _, scale = bc.case_twin(case)
    ref = bc.case_reference(case)
    worst = max(float(bc.units(f[r, b], ref[r][b], scale[r, b]).max()) for r in range(len(case.seeds)) for b in range(case.B))
    print("device against the reference, {}: {:.4g} units (tolerance {})".format(case, worst, bc.GPU_TOLERANCE_UNITS))
    assert worst <= bc.GPU_TOLERANCE_UNITS
    assert _same(res.replicates, _tree_means(f, case))
    for r in range(len(case.seeds)):
        for b in range(case.B):
            want = float(bc.reference_mean(ref[r][b]))
            assert abs(res.replicates[r, b] - want) <= U * (bc.GPU_TOLERANCE_UNITS * scale[r, b].max() + case.n) * want
    assert _same(res.prob, res.replicates.mean(axis=0))
    if len(case.seeds) == 1:
        assert np.all(np.isnan(res.stderr))
    else:
        assert _same(res.stderr, np.std(res.replicates, axis=0, ddof=1) / np.sqrt(len(case.seeds)))


@pytest.mark.parametrize("case", bc.SHAPE_CASES, ids=repr)
def test_shapes_against_the_twin(hip, case):
    res, f = _run(case)
    want, scale = bc.case_twin(case)
    assert f.shape == want.shape and np.all(np.isfinite(f)) and np.all(f >= 0)
    assert np.all(np.abs(f - want) <= U * (bc.GPU_TOLERANCE_UNITS + bc.TWIN_UNITS_OBSERVED) * scale * want)
    assert _same(res.replicates, _tree_means(f, case))
    assert res.n == case.n and np.array_equal(res.seeds, case.seeds)


def test_exact_cases(hip):
    sd = _sd()
    L = bc.chol_factor(3, 11)
    inf = np.full(3, np.inf)
    lo = np.array([[-np.inf] * 3, [-1.0, 0.3, -1.0], [-1.0, -1.0, 0.5], [np.inf, -1.0, -1.0], [-1.0, 40.0, -1.0]])
    hi = np.array([inf, [1.0, 0.3, 1.0], [1.0, 1.0, -0.5], inf, [1.0, 41.0, 1.0]])
    for n, first in ((1, 0), (63, 0), (1000, 777)):
        res, f = sd.copula_box_probabilities(L, lo, hi, n, [3, 4], first=first, return_integrand=True)
        assert np.all(f[:, 0] == 1.0) and np.all(res.replicates[:, 0] == 1.0)              # the full space
        assert np.all(f[:, 1:] == 0.0) and not np.any(np.signbit(f[:, 1:])) and np.all(res.replicates[:, 1:] == 0.0)
        # M = 1: no point, e - d exactly for any n; independent components: the product of the widths in order, at every point
        one = [sd.copula_box_probabilities([[s]], [a], [b], n, [5], shift=[m], first=first, return_integrand=True)
               for s, a, b, m in ((1.0, -1.0, 0.25, 0.0), (0.7, 0.5, np.inf, 0.1), (1.3, -np.inf, 1.5, -0.2))]
        widths = [float(r.prob[0]) for r, _ in one]
        for (r, fo), w in zip(one, widths):
            assert np.all(fo == w) and r.replicates[0, 0] == w
        res, f = sd.copula_box_probabilities(np.diag([1.0, 0.7, 1.3]), [-1.0, 0.5, -np.inf], [0.25, np.inf, 1.5], n, [5, 6],
                                             shift=[0.0, 0.1, -0.2], first=first, return_integrand=True)
        assert np.all(f == 1.0 * widths[0] * widths[1] * widths[2])
    # the upper tail through the reflection
    import mpmath
    with mpmath.workdps(40):
        tail = sd.copula_box_probabilities([[1.0]], [6.0], [np.inf], 1, [0]).prob[0]
        assert float(abs(tail - mpmath.ncdf(-6)) / mpmath.ncdf(-6)) <= bc.TAIL6_BOUND


def test_independence_and_repeatability(hip, monkeypatch):
    import torch
    sd = _sd()
    case = bc.SHAPE_CASES[4]                                                                # n = 1000, B = 37, first = 4096
    assert case.B == 37 and case.n == 1000
    res, f = _run(case)
    again, f2 = _run(case)
    assert _same(res.replicates, again.replicates) and _same(f, f2)                        # run to run
    assert _same(_run(case, return_integrand=False).replicates, res.replicates)            # with and without f_out
    _, fd = _run(case, device=True)
    assert isinstance(fd, torch.Tensor) and fd.is_cuda and fd.dtype == torch.float64 and _same(fd.cpu().numpy(), f)
    # a box alone, boxes in another order, another seed in front
    for b in (0, 17, 36):
        alone, fa = sd.copula_box_probabilities(case.L, case.lo[b], case.hi[b], case.n, case.seeds, first=case.first, return_integrand=True)
        assert _same(alone.replicates[:, 0], res.replicates[:, b]) and _same(fa[:, 0], f[:, b])
    perm = np.random.default_rng(0).permutation(case.B)
    moved = sd.copula_box_probabilities(case.L, case.lo[perm], case.hi[perm], case.n, (99,) + case.seeds, first=case.first)
    assert _same(moved.replicates[1:], res.replicates[:, perm])
    # the launch split
    for pts in ("64", "200", "4096"):
        monkeypatch.setenv("MLMC_BOX_PROB_BLOCK_POINTS", pts)
        split, fs = _run(case)
        assert _same(split.replicates, res.replicates) and _same(fs, f)
        assert _same(_run(case, return_integrand=False).replicates, res.replicates)
        _, fsd = _run(case, device=True)
        assert _same(fsd.cpu().numpy(), f)
    monkeypatch.delenv("MLMC_BOX_PROB_BLOCK_POINTS")
    # a run continued: the points of first .. first + n are those of a longer run
    _, longer = sd.copula_box_probabilities(case.L, case.lo[:3], case.hi[:3], 1500, case.seeds, first=case.first - 300, return_integrand=True)
    assert _same(longer[:, :, 300:1300], f[:, :3])


@pytest.mark.parametrize("name,L,lo,hi,exact", bc.closed_forms(), ids=[c[0] for c in bc.closed_forms()])
def test_closed_forms(hip, name, L, lo, hi, exact):
    res = _sd().copula_box_probabilities(L, lo, hi, bc.CLOSED_N, bc.SEEDS8)
    print("{}: {:.10g} exact {:.10g}, {:.2f} stderr".format(name, res.prob[0], exact, abs(res.prob[0] - exact) / res.stderr[0]))
    assert abs(res.prob[0] - exact) <= 5 * res.stderr[0]


def test_agreement_with_the_scenarios(hip, marginals):
    """a box of probability about 0.2 in the components' own units: the fraction of 2^16 scenarios of joint_samples inside it"""
    sd = _sd()
    _, distrs = marginals
    q = sd.quantiles(distrs, [np.array([0.45, 0.5]), np.array([0.1, 0.8]), np.array([0.15, 0.6])])
    lower = np.array([q[0][0], distrs[1].domain[0], q[2][0]])
    upper = np.array([np.inf, q[1][1], q[2][1]])
    res = sd.joint_probabilities(distrs, lower, upper, bc.CLOSED_N, bc.SEEDS8, corr=jc.CORR3)
    n = 2 ** 16
    x = sd.joint_samples(distrs, n, 1234, corr=jc.CORR3)
    frac = np.mean(np.all((x > lower[:, None]) & (x < upper[:, None]), axis=0))
    p = res.prob[0]
    print("box {:.6f} +- {:.2g}, scenarios {:.6f}".format(p, res.stderr[0], frac))
    assert 0.1 < p < 0.3 and abs(frac - p) <= 5 * np.sqrt(p * (1 - p) / n) + 5 * res.stderr[0]
    # by a factor, and with the unconstrained side given as the end of the domain or as inf
    F = sd.correlation_factor(jc.CORR3)[0]
    assert _same(sd.joint_probabilities(distrs, lower, upper, bc.CLOSED_N, bc.SEEDS8, factor=F).replicates, res.replicates)
    lower2 = np.array([q[0][0], -np.inf, q[2][0]])
    upper2 = np.array([distrs[0].domain[1], q[1][1], q[2][1]])
    assert _same(sd.joint_probabilities(distrs, lower2, upper2, bc.CLOSED_N, bc.SEEDS8, corr=jc.CORR3).replicates, res.replicates)


def test_conditional_against_conditional_cdfs(hip, marginals):
    """one component left: the box probability given the others is a difference of two conditional CDFs.  Both sides map the same
    scores; the device's two normcdf (16 ulp each, tests/joint_sample_cases.py), SciPy's two and the roundings of the two
    arguments stay within 64 x 2^-53 of a probability"""
    sd = _sd()
    _, distrs = marginals
    x0 = sd.quantiles([distrs[0]], [np.array([0.2, 0.5, 0.9])])[0]
    x2 = sd.quantiles([distrs[2]], [np.array([0.6, 0.3, 0.95])])[0]
    given = {0: x0, 2: x2}
    lim = sd.quantiles([distrs[1]], [np.array([0.25, 0.7])])[0]
    cdf = sd.conditional_cdfs(distrs, lim, given, jc.CORR3)                                # [3, 1, 2]
    res = sd.joint_probabilities(distrs, lim[0], lim[1], 64, [0, 1], corr=jc.CORR3, given=given)
    assert res.prob.shape == (3,) and np.all(res.stderr == 0.0)                            # M = 1: no point
    assert np.all(np.abs(res.prob - (cdf[:, 0, 1] - cdf[:, 0, 0])) <= 64 * U)
    # two components left, one of them unconstrained: the same one-dimensional problem
    g0 = {0: x0}
    wide = sd.joint_probabilities(distrs, [[lim[0], -np.inf]], [[lim[1], np.inf]], 64, [0, 1], corr=jc.CORR3, given=g0)
    cdf0 = sd.conditional_cdfs(distrs, lim, g0, jc.CORR3)                                  # [3, 2, 2]
    assert np.all(np.abs(wide.prob - (cdf0[:, 0, 1] - cdf0[:, 0, 0])) <= 64 * U)


def _raw(hip, M, L, lo, hi, seeds, n, first=0, flags=8, streams=None, shift=None, kind=0):
    L, lo, hi = (np.ascontiguousarray(v, dtype=np.float64) for v in (L, lo, hi))
    B = lo.size // max(M, 1)
    seeds = np.asarray(seeds, dtype=np.uint64)
    streams = None if streams is None else np.asarray(streams, dtype=np.uint32)
    shift = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
    mean = np.full((seeds.size, B), -7.0)
    rc = hip.lib().mlmc_copula_box_prob_batch(M, hip.ptr(L), B, hip.ptr(lo), hip.ptr(hi), hip.ptr(shift), seeds.size, hip.ptr(seeds),
                                              hip.ptr(streams), first, n, flags, hip.ptr(mean), None, kind)
    return rc, mean, hip.lib().mlmc_last_error().decode()


def test_errors_of_the_entry(hip):
    eye = np.eye(2)
    lo, hi = [-1.0, -1.0], [1.0, 1.0]
    rc, mean, _ = _raw(hip, 2, eye, lo, hi, [0], 64)
    assert rc == 0 and mean[0, 0] > 0
    big = bc.MAX_M + 1
    for kw, match in ((dict(M=big, L=np.eye(big), lo=[-1.0] * big, hi=[1.0] * big), "cap"),
                      (dict(M=0), "M < 1"),
                      (dict(L=np.diag([1.0, 0.0])), "row 1"),
                      (dict(L=np.diag([np.nan, 1.0])), "row 0"),
                      (dict(L=[[1.0, 0.0], [np.inf, 1.0]]), "row 1"),
                      (dict(lo=[-1.0, np.nan]), "box 0, component 1"),
                      (dict(lo=[-1.0, -1.0, -1.0, -1.0], hi=[1.0, 1.0, np.nan, 1.0]), "box 1, component 0"),
                      (dict(shift=[0.0, np.inf]), "shift"),
                      (dict(streams=[1024]), "coordinate 0"),
                      (dict(first=2 ** 52 - 63), "2\\^52"),
                      (dict(first=-1), "first"),
                      (dict(n=0), "n < 1"),
                      (dict(seeds=[]), "R < 1"),
                      (dict(flags=1), "ANTITHETIC"),
                      (dict(flags=9), "ANTITHETIC"),
                      (dict(flags=2), "unknown"),
                      (dict(flags=16), "unknown"),
                      (dict(kind=5), "mem_kind")):
        args = dict(M=2, L=eye, lo=lo, hi=hi, seeds=[0], n=64)
        args.update(kw)
        rc, mean, msg = _raw(hip, **args)
        import re
        assert rc != 0 and re.search(match, msg), (kw, msg)
        assert np.all(mean == -7.0)
    # the upper part of L is ignored; a stream of 1024 is fine for Philox; the last point of the sequence
    rc, m1, _ = _raw(hip, 2, [[1.0, 5.0], [0.6, 0.8]], lo, hi, [3], 64)
    rc2, m2, _ = _raw(hip, 2, [[1.0, 0.0], [0.6, 0.8]], lo, hi, [3], 64)
    assert rc == 0 and rc2 == 0 and _same(m1, m2)
    assert _raw(hip, 2, eye, lo, hi, [0], 64, flags=0, streams=[70000])[0] == 0
    assert _raw(hip, 2, eye, lo, hi, [0], 64, first=2 ** 52 - 64)[0] == 0


def test_estimate_joint_probability(hip):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.quantity.quantity import make_root_quantity
    sd = _sd()
    dev, spec, M = _small_vector_storage()
    qe.device_cache_clear()
    q = make_root_quantity(dev, spec)['q']
    doms = Estimate.estimate_domains(q, dev)
    fns = [Legendre(7, tuple(doms[m])) for m in range(M)]
    est = Estimate(q, dev, fns[0])
    pdfs = est.construct_densities(tol=1e-8, orth_moments_tol=1e-4, moments_fns=fns)
    distrs = [d[0] for d in pdfs]
    med = np.array([sd.quantiles([d], [np.array([0.5])])[0][0] for d in distrs])
    up = np.array([sd.quantiles([d], [np.array([0.9])])[0][0] for d in distrs])
    lower = np.array([[-np.inf, med[1], -np.inf, med[3]], [-np.inf, up[1], -np.inf, -np.inf]])
    upper = np.array([[np.inf, np.inf, np.inf, up[3]], [np.inf, np.inf, np.inf, med[3]]])
    # under the Pearson correlation of this storage the components move together (the second box comes out 0 and the first the
    # same for every seed), so the boxes are checked under a moderate correlation given as a matrix; corr=None is checked below
    c4 = np.full((4, 4), 0.5)
    np.fill_diagonal(c4, 1.0)
    res, ok = est.estimate_joint_probability(lower, upper, n=1024, seeds=(0, 1, 2, 3), corr=c4, densities=pdfs)
    assert res.prob.shape == (2,) and res.replicates.shape == (4, 2) and res.n == 1024 and ok.shape == (M,) and ok.dtype == bool
    assert np.all((res.prob > 0) & (res.prob < 0.5)) and np.all(res.stderr < 1e-3)
    # the unconstrained components 0 and 2 drop: the explicit two-component problem gives the same bits
    sub = sd.joint_probabilities([distrs[1], distrs[3]], lower[:, [1, 3]], upper[:, [1, 3]], 1024, (0, 1, 2, 3), corr=c4[np.ix_([1, 3], [1, 3])])
    assert _same(sub.replicates, res.replicates)
    assert _same(sd.joint_probabilities(distrs, lower, upper, 1024, (0, 1, 2, 3), corr=c4).replicates, res.replicates)
    pearson, _ = est._copula_correlation("test", None, pdfs, 1e-8, 0.0, 1e-4, fns)
    default, _ = est.estimate_joint_probability(lower, upper, n=1024, seeds=(0, 1, 2, 3), densities=pdfs)
    assert _same(default.replicates, sd.joint_probabilities(distrs, lower, upper, 1024, (0, 1, 2, 3), corr=pearson).replicates)
    # exceedance: lower = thresholds, upper = +inf; every default but the correlation
    t = np.array([-np.inf, up[1], -np.inf, med[3]])
    exc, _ = est.estimate_joint_exceedance(t, corr=c4, densities=pdfs)
    want, _ = est.estimate_joint_probability(t, np.inf, corr=c4, densities=pdfs)
    assert exc.n == 2 ** 14 and exc.replicates.shape == (8, 1) and _same(exc.replicates, want.replicates)
    assert 0 < exc.prob[0] < 0.1 + 5 * exc.stderr[0]
    # conditional on component 0
    cond, _ = est.estimate_joint_probability(lower[:1, 1:], upper[:1, 1:], n=1024, seeds=(0, 1), corr=c4, given={0: med[0]}, densities=pdfs)
    assert cond.prob.shape == (1,) and 0 < cond.prob[0] < 1
