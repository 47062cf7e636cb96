"""GPU tests of the batched max-entropy densities: mlmc_maxent_solve_batch against the single solver, batch independence,
batches larger than the CU count, argument errors, mlmc_density_eval_batch, and Estimate.construct_densities against the
loop of construct_density over the scalar components."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


def _uniform_start(R, dom):
    lam0 = np.zeros(R)
    lam0[0] = -np.log(1.0 / (dom[1] - dom[0]))
    return lam0


def _mixture(dom):
    from scipy import stats
    return lambda x: 0.6 * stats.norm(0.5, 1.0).pdf(x) + 0.4 * stats.norm(2.5, 0.7).pdf(x)


def _coop_cases():
    """(fn, mu, err, dom, lam0) of the cases of test_maxent_cooperative_launch_matches_the_step_by_step_solver"""
    from mlmc_amd import Legendre
    from mlmc_amd.tool import simple_distribution as sd
    dom = (-4.0, 6.0)
    pdf = _mixture(dom)
    out = {}
    for R, start in ((1, None), (2, None), (9, None), (21, None), (26, None), (26, "far"), (64, None), (65, None), (128, None)):
        fn = Legendre(R, dom)
        mom = sd.compute_semiexact_moments(fn, pdf)
        lam0 = _uniform_start(R, dom)
        if start == "far":
            lam0 = lam0 + 3.0 * np.sin(np.arange(R))
        out[(R, start)] = (fn, mom, np.ones(R), dom, lam0)
    return out


def _g6_cases():
    from mlmc_amd import Legendre, TransformedMoments
    g5 = np.load(os.path.join(GOLDEN, "G5_ortho.npz"))
    g6 = np.load(os.path.join(GOLDEN, "G6_maxent.npz"))
    out = {}
    for name in ("norm12", "norm110", "lognorm"):
        for R in (7, 21, 41):
            key = f"{name}_R{R}"
            dom = tuple(g5[key + "_domain"])
            fn = TransformedMoments(Legendre(R, dom), g6[key + "_L"])
            data = g6[key + "_moment_data"]
            out[key] = (fn, data[:, 0], np.sqrt(data[:, 1]), dom, _uniform_start(fn.size, dom))
    return out, g6


def _compare(single, batch, tol, tag):
    (l1, g1, h1, i1), (l2, g2, h2, i2) = single, batch
    assert i1.success == i2.success and abs(i1.nit - i2.nit) <= 1, (tag, i1.nit, i2.nit, i1.success, i2.success)
    assert i2.n_quad == i1.n_quad
    if i1.success:
        assert i2.grad_norm < tol, (tag, i2.grad_norm)
        scale = max(1.0, np.max(np.abs(l1)))
        assert np.max(np.abs(l1 - l2)) < 1e-6 * scale, (tag, np.max(np.abs(l1 - l2)))
        assert np.allclose(h2, h1, rtol=1e-6, atol=1e-9 * np.max(np.abs(h1))), tag
        assert abs(i2.moment0 - i1.moment0) <= 1e-8 * abs(i1.moment0), tag
    assert np.array_equal(h2, h2.T) and np.all(np.linalg.eigvalsh(h2) > 0), tag


@pytest.mark.parametrize("tol,max_it,n_int", [(1e-8, 100, 0), (1e-7, 100, 0), (1e-300, 7, 0), (1e-9, 100, 200)])
def test_batch_matches_single_solver(hip, tol, max_it, n_int):
    """G6 (orthogonal Legendre bases of the reference, 9 problems) and the cooperative-launch cases (R1 = 1 .. 128, a far start)
    in ONE batch with mixed R1, bases and domains, against _solve_on_device problem by problem with the same options."""
    from mlmc_amd.tool import simple_distribution as sd
    g6cases, _ = _g6_cases()
    coop = _coop_cases()
    if tol == 1e-8:
        keys = [(1, None), (2, None), (9, None), (26, None), (26, "far"), (64, None), (65, None)]
    elif tol == 1e-7:
        keys = [(128, None), (26, None), (9, None)]
    elif max_it == 7:
        keys = [(26, None), (64, None), (128, None)]
    else:
        keys = [(21, None), (9, None), (65, None)]
    cases = [coop[k] for k in keys] + list(g6cases.values())
    order = np.random.default_rng(7).permutation(len(cases))
    cases = [cases[i] for i in order]
    batch = sd._solve_batch_on_device([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases],
                                      [c[3] for c in cases], [c[4] for c in cases], tol, max_it, n_intervals=n_int)
    for k, (c, got) in enumerate(zip(cases, batch)):
        want = sd._solve_on_device(c[0], c[1], c[2], c[3], c[4], tol, max_it, n_intervals=n_int)
        _compare(want, got, tol, (k, c[0].size, tol, max_it, n_int))
        if tol > 1e-100:
            assert got[3].success == 1
        else:
            assert got[3].success == 0 and got[3].nit <= max_it


def test_batched_simple_distributions_match_reference_g6(hip):
    """estimate_densities_minimize on the G6 problems: the reference's multipliers, densities and cdf (the tolerances of
    test_orthogonal_moments_and_maxent), every OptimizeResult field as estimate_density_minimize gives it, and the batched
    density evaluation bit for bit equal to density()."""
    from mlmc_amd.tool import simple_distribution as sd
    g6cases, g6 = _g6_cases()
    batch, single = [], []
    for key, (fn, mu, err, dom, _) in g6cases.items():
        data = g6[key + "_moment_data"]
        batch.append(sd.SimpleDistribution(fn, data.copy(), domain=dom))
        single.append(sd.SimpleDistribution(fn, data.copy(), domain=dom))
    results = sd.estimate_densities_minimize(batch, tol=1e-8)
    assert len(results) == len(batch)
    for key, d, s, res in zip(g6cases, batch, single, results):
        want = s.estimate_density_minimize(tol=1e-8)
        assert res.success and res.fun_norm < 1e-8 and res.nit >= 1
        assert set(res.keys()) == set(want.keys())
        assert res.success == want.success and res.status == want.status and res.message == want.message
        assert abs(res.nit - want.nit) <= 1 and len(res.eigvals) == len(want.eigvals) and np.all(res.eigvals > 0)
        assert np.allclose(res.eigvals, want.eigvals, rtol=1e-6, atol=1e-9 * np.max(want.eigvals))
        assert np.allclose(d.multipliers, s.multipliers, rtol=1e-6, atol=1e-6)
        ref_mult = g6[key + "_sd_multipliers"]
        assert np.allclose(d.multipliers, ref_mult, rtol=2e-5, atol=2e-6), (key, np.max(np.abs(d.multipliers - ref_mult)))
        xg = g6[key + "_xgrid"]
        assert np.allclose(d.density(xg), g6[key + "_sd_density"], rtol=1e-5, atol=1e-8)
        assert np.allclose(d.cdf(xg[::8]), g6[key + "_sd_cdf"], rtol=1e-5, atol=1e-7)
    xgs = [g6[k + "_xgrid"] for k in g6cases]
    dens = sd.densities(batch, xgs)
    for d, x, got in zip(batch, xgs, dens):
        assert np.array_equal(got, d.density(x), equal_nan=True)
    common = np.linspace(-3.0, 3.0, 77)
    for d, got in zip(batch, sd.densities(batch, common)):
        assert got.shape == common.shape and np.array_equal(got, d.density(common), equal_nan=True)


def test_result_independent_of_the_batch(hip):
    """A problem alone, at position 5 of a batch of 37 and at position 30 of a permuted batch: the same bits."""
    from mlmc_amd import Legendre
    from mlmc_amd.tool import simple_distribution as sd
    g6cases, _ = _g6_cases()
    coop = _coop_cases()
    others = list(g6cases.values()) + [coop[k] for k in ((1, None), (2, None), (9, None), (26, "far"), (64, None), (128, None))]
    rng = np.random.default_rng(3)
    dom = (-3.0, 4.0)
    for i in range(36 - len(others)):
        R = int(rng.integers(3, 40))
        fn = Legendre(R, dom)
        pdf = (lambda m, s: (lambda x: np.exp(-0.5 * ((x - m) / s) ** 2) / (s * np.sqrt(2 * np.pi))))(rng.uniform(-1, 1), rng.uniform(0.6, 1.2))
        others.append((fn, sd.compute_semiexact_moments(fn, pdf), np.ones(R), dom, _uniform_start(R, dom)))
    assert len(others) == 36
    target = g6cases["lognorm_R21"]

    def run(cases):
        return sd._solve_batch_on_device([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases],
                                         [c[3] for c in cases], [c[4] for c in cases], 1e-8, 100)
    alone = run([target])[0]
    in_batch = run(others[:5] + [target] + others[5:])[5]
    perm = [others[i] for i in rng.permutation(36)]
    permuted = run(perm[:30] + [target] + perm[30:])[30]
    for got in (in_batch, permuted):
        for a, b in zip(alone[:3], got[:3]):
            assert np.array_equal(a, b)
        for f in ("nit", "success", "fun", "grad_norm", "moment0", "n_quad"):
            assert getattr(alone[3], f) == getattr(got[3], f), f


def test_batch_larger_than_the_cu_count(hip):
    """1000 problems (Gaussian mixtures of varying shape, R1 = 25) in one launch: every one converges and reproduces its
    prescribed moments."""
    from mlmc_amd import Legendre
    from mlmc_amd.tool import simple_distribution as sd
    n_cu = hip.device_info()["n_cu"]
    B, R, tol = 1000, 25, 1e-8
    assert B > n_cu
    dom = (-5.0, 5.0)
    fn = Legendre(R, dom)
    pts, w = sd._composite_gauss(dom, 256, 21)
    phi = fn.eval_all(pts)
    rng = np.random.default_rng(11)
    norm = lambda x, m, s: np.exp(-0.5 * ((x - m) / s) ** 2) / (s * np.sqrt(2 * np.pi))
    moms = []
    for _ in range(B):
        m1, m2 = rng.uniform(-1.2, 1.2, size=2)
        s1, s2 = rng.uniform(0.7, 1.3, size=2)
        p = rng.uniform(0.2, 0.8)
        moms.append((p * norm(pts, m1, s1) + (1 - p) * norm(pts, m2, s2)) * w @ phi)
    distrs = [sd.SimpleDistribution(fn, np.stack([m, np.ones(R)], axis=1), domain=dom) for m in moms]
    results = sd.estimate_densities_minimize(distrs, tol=tol)
    assert all(r.success for r in results)
    assert max(r.fun_norm for r in results) < tol
    # the moments of the solution (multipliers before the normalisation fix, result.x) are the prescribed ones: the density
    # evaluated independently of the device kernels under test, exp(clip(-phi . lambda / sigma)) in NumPy on the quadrature
    # ... and of its basis kernel: phi from the plain-NumPy recurrence of tests/maxent_exact.py
    from tests import maxent_exact as mx
    phi_host = mx.basis(mx.Desc(mx.LEGENDRE, R, dom), pts, R, np.float64)[0]
    for m, r in zip(moms, results):
        dv = np.exp(np.clip(-(phi_host @ r.x), -200, 200))
        got = (dv * w) @ phi_host
        assert np.max(np.abs(got - m)) < 50 * tol + 1e-7, np.max(np.abs(got - m))


def test_batch_argument_errors(hip):
    from mlmc_amd import Legendre
    from mlmc_amd.tool import simple_distribution as sd
    dom = (-2.0, 2.0)
    fns = [Legendre(5, dom) for _ in range(8)]
    mom = [np.eye(5)[0] for _ in range(8)]
    errs = [np.ones(5) for _ in range(8)]
    lam = [_uniform_start(5, dom) for _ in range(8)]
    doms = [dom] * 8
    bad = [e.copy() for e in errs]
    bad[5][2] = 0.0
    with pytest.raises(hip.MlmcHipError, match="problem 5.*sigma"):
        sd._solve_batch_on_device(fns, mom, bad, doms, lam, 1e-8, 100)
    big = Legendre(129, dom)
    with pytest.raises(hip.MlmcHipError, match="problem 3.*R1 = 129"):
        sd._solve_batch_on_device(fns[:3] + [big], mom[:3] + [np.eye(129)[0]], errs[:3] + [np.ones(129)], doms[:4],
                                  lam[:3] + [_uniform_start(129, dom)], 1e-8, 100)
    with pytest.raises(hip.MlmcHipError, match="problem 2.*empty domain"):
        sd._solve_batch_on_device(fns[:3], mom[:3], errs[:3], [dom, dom, (1.0, 1.0)], lam[:3], 1e-8, 100)
    # penalised options are rejected for the whole batch
    opts = hip.MaxentOpts()
    opts.tol, opts.max_it, opts.penalty_coef = 1e-8, 100, 10.0
    handles = (C.c_void_p * 1)(fns[0]._basis_handle().value)
    r1 = np.array([5], dtype=np.int32)
    a, b = np.array([dom[0]]), np.array([dom[1]])
    mu, sig, l0 = mom[0].copy(), errs[0].copy(), lam[0].copy()
    info = (hip.MaxentInfo * 1)()
    rc = hip.lib().mlmc_maxent_solve_batch(1, C.cast(handles, C.c_void_p), hip.ptr(r1), hip.ptr(a), hip.ptr(b), hip.ptr(mu),
                                           hip.ptr(sig), C.byref(opts), hip.ptr(l0), None, None, C.cast(info, C.c_void_p))
    assert rc != 0 and "penal" in hip.lib().mlmc_last_error().decode()
    with pytest.raises(hip.MlmcHipError, match="penal"):
        hip.check(rc)
    # B = 0: no-op
    assert hip.lib().mlmc_maxent_solve_batch(0, None, None, None, None, None, None, C.byref(opts), None, None, None, None) == 0
    assert sd._solve_batch_on_device([], [], [], [], [], 1e-8, 100) == []
    assert sd.estimate_densities_minimize([]) == []


def test_density_entries_share_one_workspace(hip):
    """The single entries (mlmc_density_eval, mlmc_density_integrate) use the workspace of the batched ones: whatever ran before,
    at whatever size, leaves nothing behind that a later call sees.  The smallest and the largest R1 of tests/maxent_cases.py
    (R1 = 1 and 128, plain Legendre) and the largest transformed basis (R1 = 41, orthogonalised Legendre); n = 1 and n = 257 points (grid points, both ends, points
    outside, NaN, +-inf), 257 intervals, probabilities (0.05, 0.5, 0.95).  eval with host x, eval with device x (out prefilled
    with a sentinel), eval_batch, integrate, integrate_batch, quantiles_batch and tail_means_batch, each followed by its own
    n = 0 call, run in that order and in the reverse order: every output has the same bits in both, and a device `out` is
    untouched beyond n."""
    import torch
    from mlmc_amd.tool import simple_distribution as sd
    from mlmc_amd import Legendre, TransformedMoments
    from tests import maxent_cases as mc

    class _D:
        n_intervals, _gauss_degree = 64, 21
    by_r1 = sorted(mc.cases().values(), key=lambda c: c.R1)
    picked = [by_r1[0], by_r1[-1], [c for c in by_r1 if c.desc.matrix is not None][-1]]
    assert [c.R1 for c in picked[:2]] == [1, 128] and picked[2].R1 == 41
    distrs = []
    for c in picked:
        d = _D()
        base = Legendre(c.desc.size, c.domain)
        d.moments_fn = base if c.desc.matrix is None else TransformedMoments(base, c.desc.matrix)
        d.multipliers, d._moment_errs, d.domain = mc.perturbed(c.lam0), c.sigma, c.domain
        distrs.append(d)
    probs = np.array([0.05, 0.5, 0.95])
    SENTINEL, PAD = 7.25, 64

    def eval_device(d, x):
        xd = torch.as_tensor(np.ascontiguousarray(x), device="cuda")
        od = torch.full((x.size + PAD,), SENTINEL, dtype=torch.float64, device="cuda")
        lam, sig = np.ascontiguousarray(d.multipliers), np.ascontiguousarray(d._moment_errs[:len(d.multipliers)])
        torch.cuda.synchronize()
        hip.check(hip.lib().mlmc_density_eval(d.moments_fn._basis_handle(), hip.ptr(lam), hip.ptr(sig), len(lam),
                                              hip.ptr(xd) if x.size else None, x.size, hip.ptr(od), hip.DEVICE))
        hip.check(hip.lib().mlmc_synchronize())
        got = od.cpu().numpy()
        assert np.all(got[x.size:] == SENTINEL)
        return got[:x.size]

    def integrate_batch(ivs):
        lo, hi = (np.ascontiguousarray(np.concatenate([v[k] for v in ivs])) for k in (0, 1))
        n, out = np.array([v[0].size for v in ivs], dtype=np.int64), np.empty_like(lo)
        handles, r1, lam, sig = sd._batch_problem_args(distrs)
        hip.check(hip.lib().mlmc_density_integrate_batch(len(distrs), C.cast(handles, C.c_void_p), hip.ptr(r1), hip.ptr(lam), hip.ptr(sig),
                                                         hip.ptr(lo), hip.ptr(hi), hip.ptr(n), 21, hip.ptr(out)))
        return np.split(out, np.cumsum(n)[:-1])

    def entries(n):
        """name -> call(empty): the entry on n points / intervals per problem, or on none"""
        xs = [mc.density_points(d.domain)[-n:] for d in distrs]
        iv = [tuple(v[:n] for v in mc.integrate_intervals(d.domain)) for d in distrs]
        cut = lambda arrs, empty: [a[:0] if empty else a for a in arrs]
        return {
            "eval host": lambda e: [sd._device_density(d.moments_fn, d.multipliers, d._moment_errs, x) for d, x in zip(distrs, cut(xs, e))],
            "eval device": lambda e: [eval_device(d, x) for d, x in zip(distrs, cut(xs, e))],
            "eval_batch": lambda e: sd.densities(distrs, cut(xs, e)),
            "integrate": lambda e: [sd._device_integrals(d.moments_fn, d.multipliers, d._moment_errs, *cut(v, e), 21) for d, v in zip(distrs, iv)],
            "integrate_batch": lambda e: integrate_batch([cut(v, e) for v in iv]),
            "quantiles_batch": lambda e: sd.quantiles(distrs, cut([probs] * 3, e)),
            "tail_means_batch": lambda e: [v for part in sd.tail_means(distrs, cut([probs] * 3, e)) for v in part],
        }

    def run(order):
        out = {}
        for n in order[0]:
            calls = entries(n)
            for name in (list(calls) if order[1] else list(calls)[::-1]):
                out[(name, n)] = calls[name](False)
                for v in calls[name](True)[:3]:
                    assert np.size(v) == 0, name
        return out
    first, second = run(((1, 257), True)), run(((257, 1), False))
    assert set(first) == set(second) and len(first) == 14
    for key, vals in first.items():
        assert len(vals) == len(second[key]) >= 3, key
        for a, b in zip(vals, second[key]):
            assert np.array_equal(a, b, equal_nan=True), key
    assert np.isnan(first[("eval host", 257)][0]).sum() >= 5 and np.isfinite(first[("eval host", 257)][0]).sum() >= 200
    for single, others in (("eval host", ("eval device", "eval_batch")), ("integrate", ("integrate_batch",))):
        for key in others:
            for a, b in zip(first[(single, 257)], first[(key, 257)]):
                assert a.size == 257 and np.array_equal(a, b, equal_nan=True), key


def test_host_points_beyond_the_direct_copy_threshold(hip):
    """Host point arrays of more than 1 MiB per call (Q_DIRECT_BYTES, density.hip) go to the device straight from the caller's
    memory instead of through the pinned block.  140 001 points (1.07 MiB) of a plain and a transformed basis: eval, eval_batch,
    integrate and quantiles on the whole array give the bits of the same entries on chunks of 50 000 (below the threshold), and
    eval those of device-resident points."""
    import torch
    from mlmc_amd import Legendre, TransformedMoments
    from mlmc_amd.tool import simple_distribution as sd
    from tests import maxent_cases as mc

    class _D:
        n_intervals, _gauss_degree = 64, 21
    N, CHUNK = 140001, 50000
    assert 8 * CHUNK < (1 << 20) < 8 * N
    distrs = []
    for name in ("mix_R26", "norm12_R21"):
        c, d = mc.cases()[name], _D()
        base = Legendre(c.desc.size, c.domain)
        d.moments_fn = base if c.desc.matrix is None else TransformedMoments(base, c.desc.matrix)
        d.multipliers, d._moment_errs, d.domain = mc.perturbed(c.lam0), c.sigma, c.domain
        distrs.append(d)
    chunks = lambda f, *arrs: np.concatenate([f(*[a[k:k + CHUNK] for a in arrs]) for k in range(0, N, CHUNK)])
    xs = [np.linspace(d.domain[0], d.domain[1], N) for d in distrs]
    probs = np.linspace(0.0, 1.0, N)
    for d, x, whole in zip(distrs, xs, sd.densities(distrs, xs)):
        dens = lambda v: sd._device_density(d.moments_fn, d.multipliers, d._moment_errs, v)
        want = chunks(dens, x)
        assert np.all(np.isfinite(want)) and np.array_equal(dens(x), want) and np.array_equal(whole, want)
        assert np.array_equal(sd.densities([d], [x])[0], want)
        xd = torch.as_tensor(x, device="cuda")
        od = torch.empty_like(xd)
        lam, sig = np.ascontiguousarray(d.multipliers), np.ascontiguousarray(d._moment_errs[:len(d.multipliers)])
        torch.cuda.synchronize()
        hip.check(hip.lib().mlmc_density_eval(d.moments_fn._basis_handle(), hip.ptr(lam), hip.ptr(sig), len(lam), hip.ptr(xd), N,
                                              hip.ptr(od), hip.DEVICE))
        hip.check(hip.lib().mlmc_synchronize())
        assert np.array_equal(od.cpu().numpy(), want)
        integ = lambda lo, hi: sd._device_integrals(d.moments_fn, d.multipliers, d._moment_errs, lo, hi, 21)
        lo = np.full(N, d.domain[0])
        assert np.array_equal(integ(lo, x), chunks(integ, lo, x))
        assert np.array_equal(sd.quantiles([d], [probs])[0], chunks(lambda p: sd.quantiles([d], [p])[0], probs))


# ---- Estimate.construct_densities -----------------------------------------------------------------------------------
M_TIMES, M_ARR = 2, 3          # result format: times [1, 2], one location, array (3, 1) -> M = 6 components
LOG_COMP = 4


def _vector_levels():
    """Six components of different distributions; NaNs at different samples of different components, values outside one
    component's own domain only, one strictly positive component (log moments)."""
    from tests.util import level_arrays
    steps = [0.5, 0.07, 0.01]
    levels = level_arrays([20000, 4000, 1200], steps, M_TIMES * M_ARR, 0, seed=77)
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
        f[5, 3::151] = 40.0                    # far outside component 5's own domain (under 1 %: beyond its 99th percentile)
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


def _components(st, spec):
    """q_m through the user's own indexing: m = time_index * 3 + array_index"""
    from mlmc_amd.quantity.quantity import make_root_quantity
    root = make_root_quantity(st, spec)['q']
    return root, [root[t]['0'][i, 0] for t in (1, 2) for i in range(M_ARR)]


def _check_against_loop(st, root, comps, fns, shared_fn):
    from mlmc_amd.estimator import Estimate
    est = Estimate(root, st, shared_fn)
    got = est.construct_densities(tol=1e-8, orth_moments_tol=1e-4, moments_fns=fns)
    assert len(got) == len(comps)
    xg_all = []
    for m, (q_m, (d, info, res, mobj)) in enumerate(zip(comps, got)):
        fn_m = shared_fn if fns is None else fns[m]
        d0, info0, res0, mobj0 = Estimate(q_m, st, fn_m).construct_density(tol=1e-8, orth_moments_tol=1e-4)
        assert info[1] == info0[1], m
        assert np.allclose(info[2], info0[2], rtol=1e-7, atol=1e-12), m
        assert np.allclose(info[0], info0[0], rtol=1e-7, atol=1e-14), m
        assert mobj.size == mobj0.size and res.success == res0.success, m
        assert abs(res.nit - res0.nit) <= 1, m
        scale = max(1.0, np.max(np.abs(d0.multipliers)))
        assert np.max(np.abs(d.multipliers - d0.multipliers)) < 1e-6 * scale, (m, np.max(np.abs(d.multipliers - d0.multipliers)))
        xg = np.linspace(d0.domain[0], d0.domain[1], 201)
        assert np.allclose(d.density(xg), d0.density(xg), rtol=1e-5, atol=1e-12 * np.max(d0.density(xg))), m
        xg_all.append(xg)
    return got


@pytest.mark.parametrize("chunk_size", [None, 1500])
def test_construct_densities_matches_the_loop(hip, chunk_size):
    """construct_densities over a 6-component quantity = construct_density of every scalar component (own NaN mask and
    domain clipping), once with one shared moments_fn, once with per-component moments_fns on estimate_domain (one with
    log=True)."""
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    st, spec = _vector_storage(chunk_size)
    root, comps = _components(st, spec)
    _check_against_loop(st, root, comps, None, Legendre(13, (-3.0, 3.0)))
    fns = []
    for m, q_m in enumerate(comps):
        dom = Estimate.estimate_domain(q_m, st)
        fns.append(Legendre(9 + 2 * m, dom, log=(m == LOG_COMP)))
    got = _check_against_loop(st, root, comps, fns, None)
    # the batched density evaluation of every component on one grid
    from mlmc_amd.tool import simple_distribution as sd
    xs = [np.linspace(d.domain[0], d.domain[1], 201) for d, _, _, _ in got]
    for (d, _, _, _), x, v in zip(got, xs, sd.densities([g[0] for g in got], xs)):
        assert np.array_equal(v, d.density(x), equal_nan=True)


def test_construct_densities_scalar_and_spline(hip):
    """A scalar quantity gives one entry equal to construct_density; spline moments (no linearisation) match the loop."""
    from mlmc_amd import Legendre, Spline
    from mlmc_amd.estimator import Estimate
    st, spec = _vector_storage(None)
    root, comps = _components(st, spec)
    q0 = comps[0]
    fn = Legendre(11, (-3.0, 3.0))
    got = Estimate(q0, st, fn).construct_densities(tol=1e-8)
    want = Estimate(q0, st, fn).construct_density(tol=1e-8)
    assert len(got) == 1
    d, info, res, mobj = got[0]
    assert info[1] == want[1][1] and np.allclose(info[2], want[1][2], rtol=1e-7, atol=1e-12)
    assert res.success == want[2].success
    assert np.max(np.abs(d.multipliers - want[0].multipliers)) < 1e-6 * max(1.0, np.max(np.abs(want[0].multipliers)))
    _check_against_loop(st, root, comps, None, Spline(10, (-3.0, 3.0)))
    with pytest.raises(ValueError):
        Estimate(root, st, fn).construct_densities(moments_fns=[fn, fn])


def test_per_component_pass_counts_and_sums(hip):
    """mlmc_accum_estimate_multi over a 6-component quantity (NaNs at different samples of different components, values
    outside one component's own domain, one component with log=True), chunked and unchunked Memory storages: per (level,
    component) n / n_rm exactly those of the scalar estimate of that component, sums against the NumPy oracle at 1e-10."""
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    from oracle import oracle_np as onp
    levels, _ = _vector_levels()
    for chunk_size in (None, 1500):
        st, spec = _vector_storage(chunk_size)
        root, comps = _components(st, spec)
        doms = [Estimate.estimate_domain(q_m, st) for q_m in comps]
        fns = [Legendre(13, dom, log=(m == LOG_COMP)) for m, dom in enumerate(doms)]
        exts = qe.linearized_bases(fns)
        assert exts is not None and all(e.size == 25 for e in exts)
        n, n_rm, sums = qe.multi_component_sums(root, exts)
        assert n.shape == (3, 6) and sums.shape == (3, 6, 25)
        for m, (q_m, fn) in enumerate(zip(comps, fns)):
            ref = qe.estimate_mean(qe.moments(q_m, exts[m]))
            assert np.array_equal(n[:, m], ref.n_samples) and np.array_equal(n_rm[:, m], ref.n_rm_samples), (chunk_size, m)
            b = onp.Basis(onp.LEGENDRE, 25, fn.domain, log=(m == LOG_COMP))
            chunks = []
            for l, (f, c) in enumerate(levels):
                x = f[m][:, None] if c is None else np.stack([f[m], c[m]], axis=-1)
                chunks.append([x[None]])
            oref = onp.estimate_mean(chunks, lambda x: onp.moments_rows(b, x))
            assert np.array_equal(n[:, m], oref.n_samples) and np.array_equal(n_rm[:, m], oref.n_rm_samples), (chunk_size, m)
            scale = np.sqrt(np.abs(oref.sums_sq) * oref.n_samples[:, None]) + 1e-300
            assert np.all(np.abs(sums[:, m, :] - oref.sums) <= 1e-10 * np.maximum(np.abs(oref.sums), scale)), (chunk_size, m)
    with pytest.raises(hip.MlmcHipError, match="component 1"):
        qe.multi_component_sums(root, [exts[0], fns[1]] + exts[2:])      # a family member of another size
