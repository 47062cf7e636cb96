"""GPU tests of the scenarios given a box event (mlmc_copula_box_draws_batch, the DRAWS instances of k_box_prob, and the Python
entries above it): weights and mean bit for bit those of mlmc_copula_box_prob_batch, z per point against the extended-precision
reference of tests/box_draw_cases.py within the tolerance recorded there, the bounds, u against Phi(z), independence of batch /
position / window / u_out / memory kind / launch split, repeatability, plain draws, closed-form conditional means, and
event_samples / Estimate on the mixture-marginal problem of the box-probability tests."""
import copy

import numpy as np
import pytest

from tests import box_draw_cases as dc
from tests import box_prob_cases as bc
from tests import joint_sample_cases as jc
from tests import quantile_cases as qc
from tests.test_gpu_conditional_samples import marginals  # noqa: F401  (fixture)
from tests.test_gpu_density_samples import _small_vector_storage
from tests.test_gpu_joint_samples import hip, table  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
U = bc.U


def _sd():
    from mlmc_amd.tool import simple_distribution
    return simple_distribution


def _run(case, **kw):
    args = dict(shift=case.shift, streams=case.streams, first=case.first, qmc=case.qmc)
    args.update(kw)
    return _sd().copula_box_draws(case.L, case.lo, case.hi, case.n, case.seeds, **args)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else v


def _check_u(u, z):
    """u == clamp(Phi(z)) within the normcdf allowance of tests/joint_sample_cases.py (units of 2^-53 max(Phi, 2^-53)).  Phi is
    mpmath's, as there: SciPy's ndtr is itself 22 units off at z = -3.26 (the rounding of z / sqrt 2 under erfc).  Arrays beyond 4000
    values are checked at their 1000 smallest and 1000 largest z and at 2000 values in between, evenly spaced in position."""
    u, z = np.ravel(u), np.ravel(z)
    assert np.all((u >= dc.U_LO) & (u <= dc.U_HI))
    if z.size > 4000:
        order = np.argsort(z, kind="stable")
        pick = np.unique(np.concatenate([order[:1000], order[-1000:], np.arange(0, z.size, z.size // 2000)]))
        u, z = u[pick], z[pick]
    units = jc.phi_units(u, jc.mp_ncdf(z))
    assert units.max() <= jc.phi_tolerance(), (units.max(), z[np.argmax(units)])


@pytest.mark.parametrize("case", dc.SHAPE_CASES, ids=repr)
def test_weights_and_mean_are_those_of_the_box_entry(hip, case):
    res = _run(case)
    R = len(case.seeds)
    assert res.z.shape == (R, case.B, case.M, case.n) and res.u.shape == res.z.shape and res.weights.shape == (R, case.B, case.n)
    prob, f = _sd().copula_box_probabilities(case.L, case.lo, case.hi, case.n, case.seeds, shift=case.shift,
                                             streams=None if case.streams is None else case.streams[:case.M - 1], first=case.first,
                                             qmc=case.qmc, return_integrand=True)
    assert _same(res.weights, f) and _same(res.prob.replicates, prob.replicates) and _same(res.prob.prob, prob.prob)
    assert res.prob.n == case.n and np.array_equal(res.prob.seeds, case.seeds)
    # every draw inside its box, exactly, draws of weight 0 included; the twin; u
    assert np.all(np.isfinite(res.z))
    assert np.all(res.z >= case.lo[None, :, :, None]) and np.all(res.z <= case.hi[None, :, :, None])
    _, z, _, e_z = dc.case_twin(case)
    assert np.all(np.abs(res.z - z) <= U * (dc.GPU_Z_TOLERANCE_UNITS + dc.TWIN_Z_UNITS_OBSERVED) * e_z)
    _check_u(res.u, res.z)


@pytest.mark.parametrize("case", dc.POINT_CASES, ids=repr)
def test_z_against_reference(hip, case):
    res = _run(case)
    worst = dc.worst_z_units(res.z, case)
    print("device z against the reference, {}: {:.4g} units (tolerance {})".format(case, worst, dc.GPU_Z_TOLERANCE_UNITS))
    assert worst <= dc.GPU_Z_TOLERANCE_UNITS
    assert np.all(res.z >= case.lo[None, :, :, None]) and np.all(res.z <= case.hi[None, :, :, None]) and np.all(np.isfinite(res.z))
    _check_u(res.u, res.z)


def _raw(hip, case, want_u=True, kind=0, n=None, first=None):
    """the C entry itself; arrays filled with a sentinel before the call"""
    import torch
    n = case.n if n is None else n
    first = case.first if first is None else first
    L, lo, hi = (np.ascontiguousarray(v, dtype=np.float64) for v in (case.L, case.lo, case.hi))
    seeds = np.asarray(case.seeds, dtype=np.uint64)
    streams = None if case.streams is None else np.asarray(case.streams, dtype=np.uint32)
    shift = None if case.shift is None else np.ascontiguousarray(case.shift, dtype=np.float64)
    R, B, M = seeds.size, case.B, case.M

    def array(shape, want=True):
        if not want:
            return None
        return torch.full(shape, -7.0, dtype=torch.float64, device="cuda") if kind else np.full(shape, -7.0)
    f, z, u = array((R, B, n)), array((R, B, M, n)), array((R, B, M, n), want_u)
    if kind:
        torch.cuda.synchronize()
    mean = np.full((R, B), -7.0)
    rc = hip.lib().mlmc_copula_box_draws_batch(M, hip.ptr(L), B, hip.ptr(lo), hip.ptr(hi), hip.ptr(shift), R, hip.ptr(seeds), hip.ptr(streams),
                                               first, n, 8 if case.qmc else 0, hip.ptr(mean), hip.ptr(f), hip.ptr(z), hip.ptr(u), kind)
    hip.check(rc)
    return mean, _host(f), _host(z), None if u is None else _host(u)


def test_independence_and_repeatability(hip, monkeypatch):
    import torch
    sd = _sd()
    case = dc.SHAPE_CASES[4]                                                                # n = 1000, B = 37, first = 4096
    assert case.B == 37 and case.n == 1000
    res = _run(case)
    again = _run(case)
    for a, b in zip((res.z, res.u, res.weights, res.prob.replicates), (again.z, again.u, again.weights, again.prob.replicates)):
        assert _same(a, b)                                                                 # run to run
    dev = _run(case, device=True)                                                           # device outputs
    assert all(isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float64 for v in (dev.z, dev.u, dev.weights))
    assert _same(_host(dev.z), res.z) and _same(_host(dev.u), res.u) and _same(_host(dev.weights), res.weights)
    assert _same(dev.prob.replicates, res.prob.replicates)
    for kind in (0, 1):                                                                    # without u_out
        mean, f, z, u = _raw(hip, case, want_u=False, kind=kind)
        assert u is None and _same(mean, res.prob.replicates) and _same(f, res.weights) and _same(z, res.z)
    # a box alone, boxes in another order, another seed in front
    for b in (0, 17, 36):
        alone = sd.copula_box_draws(case.L, case.lo[b], case.hi[b], case.n, case.seeds, first=case.first)
        assert _same(alone.z[:, 0], res.z[:, b]) and _same(alone.u[:, 0], res.u[:, b]) and _same(alone.weights[:, 0], res.weights[:, b])
    perm = np.random.default_rng(0).permutation(case.B)
    moved = sd.copula_box_draws(case.L, case.lo[perm], case.hi[perm], case.n, (99,) + case.seeds, first=case.first)
    assert _same(moved.z[1:], res.z[:, perm]) and _same(moved.u[1:], res.u[:, perm]) and _same(moved.weights[1:], res.weights[:, perm])
    assert _same(moved.prob.replicates[1:], res.prob.replicates[:, perm])
    # the launch split
    for pts in ("64", "128"):
        monkeypatch.setenv("MLMC_BOX_PROB_BLOCK_POINTS", pts)
        for split in (_run(case), _run(case, device=True)):
            assert _same(_host(split.z), res.z) and _same(_host(split.u), res.u) and _same(_host(split.weights), res.weights)
            assert _same(split.prob.replicates, res.prob.replicates)
        assert _same(_raw(hip, case, want_u=False)[2], res.z)
    monkeypatch.delenv("MLMC_BOX_PROB_BLOCK_POINTS")
    # a window: [50, 150) of first = 0, n = 150 against first = 50, n = 100
    for qmc in (True, False):
        long = sd.copula_box_draws(case.L, case.lo[:3], case.hi[:3], 150, case.seeds, first=0, qmc=qmc)
        part = sd.copula_box_draws(case.L, case.lo[:3], case.hi[:3], 100, case.seeds, first=50, qmc=qmc)
        assert _same(long.z[..., 50:150], part.z) and _same(long.u[..., 50:150], part.u) and _same(long.weights[..., 50:150], part.weights)


def test_plain_draws_and_exact_cases(hip):
    """the box (-inf, inf)^M: weights exactly 1 and z = L Phi^-1(w); empty boxes: weights 0, z finite and = hi in the empty
    component; a box at [40, 41]: weight 0, the draws still inside; M = 1"""
    sd = _sd()
    L = bc.chol_factor(3, 11)
    inf = np.full(3, np.inf)
    lo = np.array([-inf, [-1.0, 0.3, -1.0], [-1.0, -1.0, 0.5], [0.5, -1.0, -1.0], [-1.0, 40.0, -1.0]])
    hi = np.array([inf, [1.0, 0.3, 1.0], [1.0, 1.0, -0.5], [0.5, 1.0, 1.0], [1.0, 41.0, 1.0]])
    for n, first in ((1, 0), (63, 0), (1000, 777)):
        res = sd.copula_box_draws(L, lo, hi, n, [3, 4], first=first)
        assert np.all(res.weights[:, 0] == 1.0) and np.all(res.prob.replicates[:, 0] == 1.0)
        assert np.all(res.weights[:, 1:] == 0.0) and not np.any(np.signbit(res.weights[:, 1:])) and np.all(np.isfinite(res.z))
        for r, seed in enumerate((3, 4)):
            _, z, _, e_z = dc.twin(L, lo[0], hi[0], None, bc.points(seed, [0, 1, 2], first, n, True))
            assert np.all(np.abs(res.z[r, 0] - z) <= U * (dc.GPU_Z_TOLERANCE_UNITS + dc.TWIN_Z_UNITS_OBSERVED) * e_z)
        for b in range(1, 5):
            empty = lo[b] >= hi[b]
            assert np.all(res.z[:, b, empty] == hi[b][empty][None, :, None])
            assert np.all((res.z[:, b, ~empty] >= lo[b][~empty][None, :, None]) & (res.z[:, b, ~empty] <= hi[b][~empty][None, :, None]))
        _check_u(res.u, res.z)
        one = sd.copula_box_draws([[0.7]], [-0.2], [0.9], n, [5], shift=[0.1], first=first)
        want = sd.copula_box_probabilities([[0.7]], [-0.2], [0.9], n, [5], shift=[0.1], first=first)
        assert np.all(one.weights == want.prob[0]) and _same(one.prob.replicates, want.replicates)
        assert np.all((one.z >= -0.2) & (one.z <= 0.9)) and (n == 1 or np.ptp(one.z) > 0)


@pytest.mark.parametrize("name,lo,hi,comp,exact", dc.closed_form_events(), ids=[c[0] for c in dc.closed_form_events()])
def test_closed_forms(hip, name, lo, hi, comp, exact):
    res = _sd().copula_box_draws(dc.L2, lo, hi, bc.CLOSED_N, bc.SEEDS8)
    mean, stderr = dc.ratio_summary(res.weights[:, 0], res.z[:, 0, comp])
    print("{}: {:.8g} exact {:.8g}, {:.2f} stderr".format(name, mean, exact, abs(mean - exact) / stderr))
    assert abs(mean - exact) <= 5 * stderr


def test_errors_of_the_entry(hip):
    """the argument errors are those of the box entry (one host function); what differs: streams [M], f_out and z_out required"""
    eye = np.eye(2)
    lo, hi, seeds = np.array([-1.0, -1.0]), np.array([1.0, 1.0]), np.array([0], dtype=np.uint64)
    mean, f, z = np.full((1, 1), -7.0), np.full((1, 1, 64), -7.0), np.full((1, 1, 2, 64), -7.0)

    def call(M=2, L=eye, streams=None, flags=8, f=f, z=z, n=64, kind=0):
        st = None if streams is None else np.asarray(streams, dtype=np.uint32)
        rc = hip.lib().mlmc_copula_box_draws_batch(M, hip.ptr(np.ascontiguousarray(L, dtype=np.float64)), 1, hip.ptr(lo), hip.ptr(hi), None, 1,
                                                   hip.ptr(seeds), hip.ptr(st), 0, n, flags, hip.ptr(mean), hip.ptr(f), hip.ptr(z), None, kind)
        return rc, hip.lib().mlmc_last_error().decode()
    import re
    for kw, match in ((dict(streams=[0, 1024]), "coordinate 1"), (dict(f=None), "null"), (dict(z=None), "null"), (dict(M=0), "M < 1"),
                      (dict(L=np.diag([1.0, 0.0])), "row 1"), (dict(flags=1), "ANTITHETIC"), (dict(n=0), "n < 1"), (dict(kind=5), "mem_kind")):
        rc, msg = call(**kw)
        assert rc != 0 and re.search(match, msg) and "mlmc_copula_box_draws_batch" in msg, (kw, msg)
        assert np.all(mean == -7.0) and np.all(z == -7.0)
    assert call(streams=[0, 1023])[0] == 0 and call(streams=[0, 70000], flags=0)[0] == 0 and np.all(z != -7.0)


# ---- event_samples and Estimate on the mixture marginals ------------------------------------------------------------------------
def _event_box(sd, distrs):
    """the box of probability about 0.2 of tests/test_gpu_box_prob.py"""
    q = sd.quantiles(distrs, [np.array([0.45, 0.5]), np.array([0.1, 0.8]), np.array([0.15, 0.6])])
    return np.array([q[0][0], distrs[1].domain[0], q[2][0]]), np.array([np.inf, q[1][1], q[2][1]])


def _cdf_violation(pr, x, lower, upper, z_lo, z_hi):
    """(violation, allowance) in CDF space of draws x of one marginal against its limits: Fhat_ref(lower) - Fhat_ref(x) (likewise
    above).  Allowed: what tests/quantile_cases.py allows the quantile entry at x (quantile_tolerance units of 2^-53 (scale + p)
    and the resolution of x, 4 rho spacing(x) / T), the same again for the CDF entry that mapped the limit, and the allowances of
    tests/joint_sample_cases.py for the normcdfinv and the normcdf between the two"""
    ref, tol = qc.RuleTable(pr["case"], pr["lam"], pr["quad"]), qc.quantile_tolerance(pr["case"])
    F, sc = ref.fhat(x)
    slack = 4 * ref.density(x) * np.spacing(np.abs(x)) / ref.T
    viol, allow = np.zeros(x.shape), np.zeros(x.shape)
    for lim, zl, sign in ((lower, z_lo, 1.0), (upper, z_hi, -1.0)):
        if not np.isfinite(zl):
            continue
        Fl, scl = ref.fhat(np.array([lim]))
        viol = np.maximum(viol, (sign * (Fl[0] - F)).astype(np.float64))
        phi = np.exp(-0.5 * zl * zl) / np.sqrt(2 * np.pi)
        allow = np.maximum(allow, (U * (tol * (sc + F) + tol * (scl[0] + Fl[0]) + jc.z_tolerance() * max(1.0, abs(zl)) * phi
                                        + jc.phi_tolerance() * Fl[0]) + slack).astype(np.float64))
    return viol, allow


def test_event_samples(hip, marginals):
    sd = _sd()
    group, distrs = marginals
    lower, upper = _event_box(sd, distrs)
    ev = sd.event_samples(distrs, lower, upper, bc.CLOSED_N, bc.SEEDS8, corr=jc.CORR3)
    R, n = len(bc.SEEDS8), bc.CLOSED_N
    assert ev.draws.shape == (R, 1, 3, n) and ev.weights.shape == (R, 1, n) and ev.ess.shape == (R, 1) and np.all(ev.ok)
    # draws == quantiles(distrs, u), bit for bit
    want = sd.quantiles(distrs, [np.ascontiguousarray(ev.uniforms[:, :, m, :]) for m in range(3)])
    for m in range(3):
        assert _same(ev.draws[:, :, m, :], want[m])
    assert _same(ev.ess, dc.ess(ev.weights)) and np.all((ev.ess > 0.2 * n) & (ev.ess <= n))
    # every draw of positive weight lies within its limits, up to the accuracy of the quantile entry
    z_lim = sd.normal_scores([distrs[0], distrs[2], distrs[1], distrs[2]], np.array([[lower[0]], [lower[2]], [upper[1]], [upper[2]]]))[:, 0]
    z_lo, z_hi = np.array([z_lim[0], -np.inf, z_lim[1]]), np.array([np.inf, z_lim[2], z_lim[3]])
    pos = (ev.weights[:2, 0] > 0).ravel()                    # two seeds: the long-double reference is slow
    assert pos.any()
    for m in range(3):
        x = ev.draws[:2, 0, m].ravel()[pos]
        viol, allow = _cdf_violation(group[m], x, lower[m], upper[m], z_lo[m], z_hi[m])
        print("component {}: {} of {} draws beyond a limit, largest violation {:.3g} (allowed there {:.3g})".format(
            m, int(np.sum(viol > 0)), x.size, viol.max(), allow[np.argmax(viol)]))
        assert np.all(viol <= allow)
    # the probability, and the means against the scenarios of joint_samples that fall inside the event
    joint = sd.joint_probabilities(distrs, lower, upper, bc.CLOSED_N, bc.SEEDS8, corr=jc.CORR3)
    p = ev.prob.prob[0]
    assert 0.1 < p < 0.3 and abs(p - joint.prob[0]) <= 5 * joint.stderr[0]
    x = sd.joint_samples(distrs, 2 ** 16, 1234, corr=jc.CORR3)
    inside = np.all((x > lower[:, None]) & (x < upper[:, None]), axis=0)
    kept = x[:, inside]
    mean, stderr = ev.means()
    rej, rej_err = kept.mean(axis=1), kept.std(axis=1, ddof=1) / np.sqrt(kept.shape[1])
    print("event means {} +- {}, rejection ({} scenarios) {} +- {}".format(mean[0], stderr[0], kept.shape[1], rej, rej_err))
    assert mean.shape == (1, 3) and np.all(np.abs(mean[0] - rej) <= 5 * np.hypot(stderr[0], rej_err))
    wq = ev.weighted_quantiles([0.5])
    assert wq.shape == (1, 3, 1) and np.all(np.abs(wq[0, :, 0] - np.median(kept, axis=1)) <= 0.05 * (kept.max(axis=1) - kept.min(axis=1)))
    # by a factor; device tensors hold the same bits and the host methods refuse them
    F = sd.correlation_factor(jc.CORR3)[0]
    assert _same(sd.event_samples(distrs, lower, upper, 256, (1, 2), factor=F).draws,
                 sd.event_samples(distrs, lower, upper, 256, (1, 2), corr=jc.CORR3).draws)
    dev = sd.event_samples(distrs, lower, upper, bc.CLOSED_N, bc.SEEDS8, corr=jc.CORR3, device=True)
    assert dev.draws.is_cuda and _same(_host(dev.draws), ev.draws) and _same(_host(dev.weights), ev.weights) and _same(dev.ess, ev.ess)
    assert _same(_host(dev.uniforms), ev.uniforms)
    with pytest.raises(ValueError, match="copy"):
        dev.means()


def test_event_samples_order_and_degenerate_component(hip, marginals):
    """only component 0 constrained: constant weights whatever the caller's order, rows in the caller's order; a component without
    a positive finite mass is a NaN row with ok false, the other rows are unaffected"""
    sd = _sd()
    _, distrs = marginals
    t = sd.quantiles([distrs[0]], [np.array([0.9])])[0][0]
    lower = np.array([t, -np.inf, -np.inf])
    n = 1024
    ev = sd.event_samples(distrs, lower, np.inf, n, (0, 1), corr=jc.CORR3)
    assert np.all(ev.weights == ev.weights[0, 0, 0]) and np.all(np.abs(ev.ess - n) <= 1e-9 * n)
    med0 = sd.quantiles([distrs[0]], [np.array([0.5])])[0][0]                  # the limits themselves: test_event_samples
    assert abs(ev.prob.prob[0] - 0.1) <= 1e-6 and np.all(ev.draws[:, 0, 0] > med0)
    for perm in ((1, 0, 2), (1, 2, 0)):                       # the same chain (0, 1, 2): the same draws, row by row
        perm = np.array(perm)
        moved = sd.event_samples([distrs[m] for m in perm], lower[perm], np.inf, n, (0, 1), corr=jc.CORR3[np.ix_(perm, perm)])
        assert _same(moved.draws, ev.draws[:, :, perm]) and _same(moved.weights, ev.weights) and _same(moved.uniforms, ev.uniforms[:, :, perm])
    moved = sd.event_samples([distrs[m] for m in (2, 1, 0)], lower[::-1], np.inf, n, (0, 1), corr=jc.CORR3[::-1, ::-1])
    assert np.all(moved.weights == moved.weights[0, 0, 0]) and np.all(moved.draws[:, 0, 2] > med0)   # chain (0, 2, 1)
    # streams belong to chain positions
    st = sd.event_samples(distrs, lower, np.inf, n, (0, 1), corr=jc.CORR3, streams=[5, 1, 2])
    assert _same(st.draws[:, :, 1:], ev.draws[:, :, 1:]) is False and _same(st.weights, ev.weights)
    # a mass that is not finite: a domain that reaches outside the domain of the moments, where the density is NaN
    # (tests/test_gpu_quantiles.py)
    bad = copy.copy(distrs[2])
    a, b = distrs[2].domain
    bad.domain = (a - (b - a), b)
    deg = sd.event_samples([distrs[0], distrs[1], bad], lower, np.inf, n, (0, 1), corr=jc.CORR3)
    assert deg.ok.tolist() == [True, True, False] and np.all(np.isnan(deg.draws[:, :, 2]))
    assert _same(deg.draws[:, :, :2], ev.draws[:, :, :2]) and _same(deg.weights, ev.weights) and _same(deg.uniforms, ev.uniforms)
    m, _ = deg.means()
    assert np.isnan(m[0, 2]) and np.all(np.isfinite(m[0, :2]))


def test_event_samples_given(hip, marginals):
    """given component 1: its rows hold the given values; with nothing constrained the other rows are the draws of
    conditional_samples on the same Sobol' points (weights exactly 1), up to the rounding of the factor and of the sum:
    the factor is the Cholesky factor of F_c F_c^T, equal to F_c within a few ulp, |y| <= 8.3, and each side takes one normcdf
    (16 units, tests/joint_sample_cases.py): 2^-44 of a probability covers it, a wrong shift is an error of 1e-2"""
    sd = _sd()
    _, distrs = marginals
    x1 = sd.quantiles([distrs[1]], [np.array([0.2, 0.5, 0.93])])[0]
    given = {1: x1}
    n = 512
    free = sd.event_samples(distrs, -np.inf, np.inf, n, (7,), corr=jc.CORR3, given=given)
    assert free.draws.shape == (1, 3, 3, n) and np.all(free.weights == 1.0) and np.all(free.prob.prob == 1.0)
    assert np.array_equal(free.draws[0, :, 1], np.tile(x1[:, None], (1, n)))
    x, u = sd.conditional_samples(distrs, n, 7, given, corr=jc.CORR3, qmc=True, return_uniforms=True)
    assert np.all(np.abs(free.uniforms[0] - u) <= 2.0 ** -44)
    assert _same(free.uniforms[0, :, 1], u[:, 1])
    # constrained as well: inside the event, the given rows unchanged, probability below 1 and different per set
    t = sd.quantiles([distrs[0]], [np.array([0.7])])[0][0]
    ev = sd.event_samples(distrs, [t, -np.inf, -np.inf], np.inf, n, (7, 8), corr=jc.CORR3, given=given)
    assert ev.draws.shape == (2, 3, 3, n) and np.array_equal(ev.draws[1, :, 1], np.tile(x1[:, None], (1, n)))
    med0 = sd.quantiles([distrs[0]], [np.array([0.5])])[0][0]
    assert np.all(ev.draws[:, :, 0] > med0) and np.all((ev.prob.prob > 0) & (ev.prob.prob < 1))
    cond = sd.joint_probabilities(distrs, [[t, -np.inf]], [[np.inf, np.inf]], n, (7, 8), corr=jc.CORR3, given=given)
    assert np.all(np.abs(ev.prob.prob - cond.prob) <= 64 * U) and np.all(np.diff(ev.prob.prob) > 0)      # CORR3[0, 1] = 0.8


def test_estimate_event_means(hip):
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
    c4 = np.full((4, 4), 0.5)
    np.fill_diagonal(c4, 1.0)
    t = np.array([-np.inf, up[1], -np.inf, med[3]])
    res, ok = est.estimate_event_means(t, np.inf, n=1024, seeds=(0, 1, 2, 3), corr=c4, densities=pdfs)
    want = sd.event_samples(distrs, t, np.inf, 1024, (0, 1, 2, 3), corr=c4)
    mean, stderr = want.means()
    assert ok.shape == (M,) and res.mean.shape == (1, M) and _same(res.mean, mean) and _same(res.stderr, stderr)
    assert _same(res.prob.replicates, want.prob.replicates) and _same(res.ess, want.ess)
    exc, _ = est.estimate_joint_exceedance(t, n=1024, seeds=(0, 1, 2, 3), corr=c4, densities=pdfs)
    assert np.all(np.abs(res.prob.prob - exc.prob) <= 5 * np.hypot(res.prob.stderr, exc.stderr) + 64 * U)
    assert res.mean[0, 1] > up[1] and res.mean[0, 3] > med[3]
    scen, _ = est.sample_given_event(1024, t, np.inf, seeds=(0, 1, 2, 3), corr=c4, densities=pdfs)
    assert _same(scen.draws, want.draws) and _same(scen.weights, want.weights)
    dscen, _ = est.sample_given_event(64, t, np.inf, seeds=(0,), corr=c4, densities=pdfs, device=True)
    assert dscen.draws.is_cuda and _same(_host(dscen.draws), est.sample_given_event(64, t, np.inf, seeds=(0,), corr=c4, densities=pdfs)[0].draws)
