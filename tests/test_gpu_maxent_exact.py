"""GPU tests of the max-entropy kernels against the extended-precision reference of tests/maxent_exact.py.

Every output of a solve -- info.fun, grad_out, hess_out, info.moment0, info.grad_norm, the verdict `success` -- is compared with
the functional evaluated in 80-bit long double AT THE MULTIPLIERS THE DEVICE RETURNED, on the library's own quadrature, through
each of the three solver routes (cooperative single launch, step by step, batched).  Densities and interval integrals are
compared the same way at converged, perturbed and clipping multipliers.  Errors are measured in units of u * scale (u = 2^-53,
scale = the first-order condition scale of the quantity); the tolerance is 4 x the worst error of a plain-fp64 evaluation of
the same sums (mc.TWIN_UNITS, calibrated on the CPU by tests/test_maxent_exact_cpu.py), at least 16 units.  Every test prints
the worst units it saw per quantity before it asserts (pytest -s)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle_np as onp
from tests import maxent_cases as mc
from tests import maxent_exact as mx

pytestmark = pytest.mark.gpu
LD = np.longdouble
U = 2.0 ** -53
ROUTES = ("coop", "stepwise", "batch")
RESOLVING = ((64, 21), (200, 21))      # the rules that resolve every basis of the table


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


_FNS = {}


def _fn(case):
    """the package's moments object of a case; its transform constants are the ones the reference uses"""
    if case.name not in _FNS:
        import mlmc_amd
        d = case.desc
        cls = {mx.LEGENDRE: mlmc_amd.Legendre, mx.MONOMIAL: mlmc_amd.Monomial, mx.FOURIER: mlmc_amd.Fourier, mx.SPLINE: mlmc_amd.Spline}[d.kind]
        base = cls(d.size, d.domain, ref_domain=d.ref_domain, log=d.log)
        assert float(base._linear_scale) == d.scale and float(base._linear_shift) == d.shift
        _FNS[case.name] = base if d.matrix is None else mlmc_amd.TransformedMoments(base, d.matrix)
        assert _FNS[case.name].size == d.out_size
    return _FNS[case.name]


def _solve_single(case, quad, tol, max_it, stepwise):
    from mlmc_amd.tool import simple_distribution as sd
    if stepwise:
        os.environ["MLMC_MAXENT_STEPWISE"] = "1"
    try:
        return sd._solve_on_device(_fn(case), case.mu, case.sigma, case.domain, case.lam0, tol, max_it, n_intervals=quad[0],
                                   gauss_degree=quad[1])
    finally:
        os.environ.pop("MLMC_MAXENT_STEPWISE", None)


def _solve_batch(hip, cases, quad, tol, max_it):
    """mlmc_maxent_solve_batch on the raw arrays (the padding of the outputs is checked too); grad / hess are pre-filled with
    a sentinel so that entries the kernel does not write show"""
    B = len(cases)
    r1 = np.array([c.R1 for c in cases], dtype=np.int32)
    ldv = int(r1.max())
    mu, sig, lam = np.zeros((B, ldv)), np.ones((B, ldv)), np.zeros((B, ldv))
    for b, c in enumerate(cases):
        mu[b, :c.R1], sig[b, :c.R1], lam[b, :c.R1] = c.mu[:c.R1], c.sigma[:c.R1], c.lam0
    lo = np.ascontiguousarray([c.domain[0] for c in cases])
    hi = np.ascontiguousarray([c.domain[1] for c in cases])
    opts = hip.MaxentOpts()
    opts.tol, opts.max_it, opts.n_intervals, opts.gauss_degree = float(tol), int(max_it), int(quad[0]), int(quad[1])
    handles = (C.c_void_p * B)(*[_fn(c)._basis_handle().value for c in cases])
    infos = (hip.MaxentInfo * B)()
    grad = np.full((B, ldv), 7.25)
    hess = np.full((B, ldv, ldv), 7.25)
    hip.check(hip.lib().mlmc_maxent_solve_batch(B, C.cast(handles, C.c_void_p), hip.ptr(r1), hip.ptr(lo), hip.ptr(hi), hip.ptr(mu),
                                                hip.ptr(sig), C.byref(opts), hip.ptr(lam), hip.ptr(grad), hip.ptr(hess),
                                                C.cast(infos, C.c_void_p)))
    out = []
    for b, c in enumerate(cases):
        r = c.R1
        pad_g, pad_h = grad[b, r:], np.concatenate([hess[b, r:, :].ravel(), hess[b, :r, r:].ravel()])
        assert np.all(pad_g == 0.0) and np.all(pad_h == 0.0), (c.name, "entries beyond R1 are not zero")
        out.append((lam[b, :r].copy(), grad[b, :r].copy(), hess[b, :r, :r].copy(), infos[b]))
    return out


class Worst:
    """worst units per (route, quantity), and where"""

    def __init__(self):
        self.w = {}

    def add(self, route, quantity, value, where, case):
        quantity = f"{quantity}/{mc.tolerance_class(case)}"      # one line per tolerance class
        if value > self.w.get((route, quantity), (-1.0, None))[0]:
            self.w[(route, quantity)] = (value, where)

    def report(self, title):
        print()
        for (route, q), (v, where) in sorted(self.w.items()):
            print(f"{title}: worst {q:17s} {route:9s} {v:10.4g} units at {where}")


def _norm(v):
    return np.sqrt(np.sum(np.asarray(v, dtype=LD) ** 2))


def _check_solution(case, quad, tol, max_it, route, sol, worst, failures, require_success):
    lam, grad, hess, info = sol
    a, b = case.domain
    where = f"{case.name} {quad[0]}x{quad[1]} tol {tol:g} max_it {max_it}"
    ref = mx.functional_ld(case.desc, case.mu, case.sigma, lam, a, b, *quad)
    mc.assert_clip_band(ref["e"])
    worst.add(route, "u*c_max", U * float(ref["c_max"]), where + " (not units: the scales are first-order while this is << 1)", case)
    got = dict(F=(info.fun, ref["F"], ref["F_scale"]), g=(grad, ref["g"], ref["g_scale"]), H=(hess, ref["H"], ref["H_scale"]),
               moment0=(info.moment0, ref["moment0"], ref["m_scale"]))
    tol_g = mc.device_tolerance(case, "g")
    for q, (val, want, scale) in got.items():
        un = mx.units(val, want, scale)
        worst.add(route, q, un, where, case)
        if not un <= mc.device_tolerance(case, q):
            failures.append(f"{route} {where}: {q} is {un:.4g} units off (tolerance {mc.device_tolerance(case, q):g})")
    if not np.array_equal(hess, hess.T):
        failures.append(f"{route} {where}: hess_out is not symmetric")
    if info.n_quad != quad[0] * quad[1] or not (0 <= info.nit <= max_it):
        failures.append(f"{route} {where}: n_quad {info.n_quad}, nit {info.nit}")
    # the reported gradient norm and the verdict
    gn = _norm(ref["g"])
    bound = float(_norm(tol_g * U * ref["g_scale"]) + 8 * U * gn)
    gn = float(gn)
    worst.add(route, "grad_norm", abs(info.grad_norm - gn) / bound if bound > 0 else 0.0, where + " (in bounds)", case)
    if not abs(info.grad_norm - gn) <= bound:
        failures.append(f"{route} {where}: grad_norm {info.grad_norm:.17g}, reference {gn:.17g}, bound {bound:.3g}")
    if info.success == 1 and not gn < tol + bound:
        failures.append(f"{route} {where}: success but the reference gradient norm is {gn:.3g}")
    if tol < 1e-100 and info.success == 0 and not gn >= tol:
        failures.append(f"{route} {where}: no success on a capped solve, but the reference gradient norm is {gn:.3g}")
    if tol < 1e-100 and info.success == 1 and not info.grad_norm == 0.0:
        # a device gradient that is exactly zero (R1 = 1, 2: reached within the cap) is the only way below 1e-300
        failures.append(f"{route} {where}: success on a capped solve with grad_norm {info.grad_norm:.3g}")
    if require_success:
        if not (info.success == 1 and gn < tol):
            failures.append(f"{route} {where}: not converged: success {info.success}, reference gradient norm {gn:.3g}")
    if require_success and quad in RESOLVING:
        # on a rule four times finer: the moments of the returned density against mu, next to the discretisation error the
        # reference itself measures for this problem (difference of its gradients between the two rules)
        fine = mx.functional_ld(case.desc, case.mu, case.sigma, lam, a, b, 4 * quad[0], quad[1], hess=False)
        disc, gfine = float(_norm(fine["g"] - ref["g"])), float(_norm(fine["g"]))
        worst.add(route, "disc/tol", disc / tol, where, case)
        if case.group in ("g6", "mixture"):
            if not (disc < tol and gfine < 2 * tol):
                failures.append(f"{route} {where}: discretisation error {disc:.3g}, fine-rule residual {gfine:.3g}")
    return ref


def _expect_convergence(case, quad):
    """Convergence is REQUIRED on the two rules that resolve every basis of the table (64 x 21 and 200 x 21).  On a coarser rule
    it is required where the rule has at least four nodes per moment and the fp64 twin's own Newton iteration converges; below
    that the Hessian is (nearly) singular and whether a minimiser exists is a property of the rule, not of the solver.  The
    outputs are checked against the reference at the returned multipliers in every case."""
    if quad in RESOLVING:
        return True
    if quad[0] * quad[1] < 4 * case.R1:
        return False
    lam = mc.newton_f64(case, quad, tol=1e-10)
    f = mx.functional_ld(case.desc, case.mu, case.sigma, lam, *case.domain, *quad, hess=False)
    return bool(_norm(f["g"]) < 1e-10)


SWEEPS = [(q, mc.STOPPING[0]) for q in mc.QUADRATURES] + [(mc.DEFAULT_QUAD, s) for s in mc.STOPPING[1:]] + \
         [(q, mc.STOPPING[2]) for q in mc.QUADRATURES[1:]]


@pytest.mark.parametrize("quad,stop", SWEEPS, ids=[f"{q[0]}x{q[1]}-tol{s[0]:g}-it{s[1]}" for q, s in SWEEPS])
def test_solver_outputs_against_the_reference(hip, quad, stop):
    """Every case of the table on one quadrature and one stopping rule, through the three routes (the batch shuffled):
    F, gradient, Hessian, moment0 within the tolerance of their condition scale at the returned multipliers; Hessian exactly
    symmetric; batch padding exactly zero; grad_norm within the propagated bound; an honest verdict; convergence where the
    problem is resolved, with the discretisation error measured by the reference on a four times finer rule.
    All quadratures are run to convergence (problems with fewer nodes than moments excepted, mc.on_rule) and under the
    iteration cap 3 (every problem, R1 > Q included); the caps 1 and 7 on the default rule."""
    tol, max_it = stop
    cases = mc.on_rule_cases(quad, to_convergence=tol > 1e-100)
    assert len(cases) == (27 if tol < 1e-100 or quad[0] * quad[1] >= 128 else {(1, 5): 14, (1, 21): 24, (7, 5): 21}[quad]), len(cases)
    order = np.random.default_rng(quad[0] * 100 + max_it).permutation(len(cases))
    shuffled = [cases[i] for i in order]
    batch = dict(zip([c.name for c in shuffled], _solve_batch(hip, shuffled, quad, tol, max_it)))
    worst, failures = Worst(), []
    for c in cases:
        need = tol > 1e-100 and _expect_convergence(c, quad)
        for route in ROUTES:
            sol = batch[c.name] if route == "batch" else _solve_single(c, quad, tol, max_it, route == "stepwise")
            _check_solution(c, quad, tol, max_it, route, sol, worst, failures, need)
    worst.report(f"solve {quad[0]}x{quad[1]} tol {tol:g} max_it {max_it}")
    print("\n".join(failures))
    assert not failures, f"{len(failures)} findings, first: {failures[0]}"


def test_line_search_give_up_returns_the_hessian_of_the_returned_multipliers(hip):
    """mc.give_up_case: no step length passes the Armijo test (shown on the reference by test_give_up_start_admits_no_step),
    the first diagonal shift 1e-8 (1 + |F|) already exceeds 1e20, so every route gives up after one line search and returns
    the start: nit = 0, success = 0, the multipliers bit for bit.  The cooperative and the batched kernel have by then
    overwritten their sums with those of the rejected trial point lambda + p; gradient, F, moment0 AND the Hessian must still
    be those of the returned multipliers (the Hessian at lambda + p is 1e5 units away)."""
    c = mc.give_up_case()
    quad, tol, max_it = mc.DEFAULT_QUAD, 1e-8, 100
    worst, failures = Worst(), []
    sols = dict(coop=_solve_single(c, quad, tol, max_it, False), stepwise=_solve_single(c, quad, tol, max_it, True),
                batch=_solve_batch(hip, [mc.cases()["mix_R9"], c], quad, tol, max_it)[1])
    for route, sol in sols.items():
        assert np.array_equal(sol[0], c.lam0) and sol[3].nit == 0 and sol[3].success == 0, (route, sol[0], sol[3].nit, sol[3].success)
        _check_solution(c, quad, tol, max_it, route, sol, worst, failures, False)
    worst.report("give-up exit")
    print("\n".join(failures))
    assert not failures, f"{len(failures)} findings, first: {failures[0]}"


# ---------------------------------------------------------------------------------------------------------------------------
# densities and interval integrals
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def converged(hip):
    """name -> multipliers of the cooperative solve on the default rule (tol 1e-8)"""
    out = {}
    for c in mc.cases().values():
        lam, _, _, info = _solve_single(c, mc.DEFAULT_QUAD, 1e-8, 100, False)
        assert info.success == 1, c.name
        out[c.name] = lam
    return out


def _oracle_density(case, lam, x):
    """NaN positions of onp.MaxEntOracle.density"""
    kinds = {mx.LEGENDRE: onp.LEGENDRE, mx.MONOMIAL: onp.MONOMIAL, mx.FOURIER: onp.FOURIER, mx.SPLINE: onp.SPLINE}
    d = case.desc
    ob = onp.Basis(kinds[d.kind], d.size, d.domain, d.ref_domain, d.log, True, d.matrix)
    o = onp.MaxEntOracle(ob, np.stack([case.mu, case.sigma ** 2], axis=1), case.domain)
    o.multipliers = np.asarray(lam, dtype=np.float64)
    with np.errstate(all="ignore"):
        return o.density(x)


def _density_routes(hip, case, lam, x):
    """mlmc_density_eval with host x, with device x, and mlmc_density_eval_batch (two problems, this one second)"""
    import torch
    from mlmc_amd.tool import simple_distribution as sd
    fn = _fn(case)
    host = sd._device_density(fn, lam, case.sigma, x)
    xd = torch.as_tensor(np.ascontiguousarray(x), device="cuda")
    od = torch.full_like(xd, 7.25)
    lam_c, sig_c = np.ascontiguousarray(lam, dtype=np.float64), np.ascontiguousarray(case.sigma[:len(lam)])
    hip.check(hip.lib().mlmc_density_eval(fn._basis_handle(), hip.ptr(lam_c), hip.ptr(sig_c), len(lam_c), hip.ptr(xd), x.size,
                                          hip.ptr(od), hip.DEVICE))
    hip.check(hip.lib().mlmc_synchronize())
    dev = od.cpu().numpy()

    class _D:
        pass
    d = _D()
    d.moments_fn, d.multipliers, d._moment_errs = fn, lam_c, case.sigma
    other = mc.cases()["mix_R128" if case.name != "mix_R128" else "mix_R2"]
    o = _D()
    o.moments_fn, o.multipliers, o._moment_errs = _fn(other), other.lam0, other.sigma
    batch = sd.densities([o, d], [np.linspace(other.domain[0], other.domain[1], 3), x])[1]
    return dict(host=host, device=dev, batch=batch)


def test_density_eval_against_the_reference(hip, converged):
    """mlmc_density_eval (host and device x) and mlmc_density_eval_batch at the converged and at perturbed multipliers of every
    case: a 1001-point grid, both end points, nextafter outside each end, far outside, NaN, +-inf, -0.0; prefixes of
    n = 1, 255, 256, 257 points.  NaN positions are the fp64 oracle's, values within the tolerance of rho(x) c(x)."""
    worst, failures = Worst(), []
    for c in mc.cases().values():
        x = mc.density_points(c.domain)
        for tag, lam in (("converged", converged[c.name]), ("perturbed", mc.perturbed(converged[c.name]))):
            ref, scale, e = mx.density_ld(c.desc, lam, c.sigma, x)
            mc.assert_clip_band(e)
            assert np.array_equal(np.isnan(ref), np.isnan(_oracle_density(c, lam, x))), c.name
            assert np.sum(np.isnan(ref)) >= 5 and np.sum(~np.isnan(ref)) >= 1001
            got = _density_routes(hip, c, lam, x)
            for n in (1, 255, 256, 257):
                for route, val in _density_routes(hip, c, lam, x[500:500 + n]).items():
                    got[f"{route} n={n}"] = val
            for route, val in got.items():
                sl = slice(500, 500 + int(route.split("=")[1])) if "=" in route else slice(None)
                un = mx.units(val, ref[sl], scale[sl])
                worst.add(route.split(" ")[0], "density", un, f"{c.name} {tag}", c)
                if not un <= mc.device_tolerance(c, "density"):
                    failures.append(f"{route} {c.name} {tag}: density {un:.4g} units off (tolerance {mc.device_tolerance(c, 'density'):g})")
    worst.report("density")
    print("\n".join(failures))
    assert not failures, f"{len(failures)} findings, first: {failures[0]}"


def test_density_clip(hip, converged):
    """multipliers scaled so that the exponent passes +200 at some points and -200 at others: those outputs are exp(+-200)
    exactly as NumPy rounds it; the others within the tolerance.  No reference exponent lies within 1e-9 of a bound."""
    worst = Worst()
    for name in mc.CLIP_CASES:
        c = mc.cases()[name]
        x = mc.density_points(c.domain)
        lam = mc.clip_multipliers(c, converged[name])
        ref, scale, e = mx.density_ld(c.desc, lam, c.sigma, x)
        mc.assert_clip_band(e)
        fin = np.isfinite(e)
        hi_, lo_ = fin & (e > 200), fin & (e < -200)
        assert hi_.any() and lo_.any() and (fin & (np.abs(e) < 200)).any()
        for route, val in _density_routes(hip, c, lam, x).items():
            assert np.all(val[hi_] == np.exp(200.0)) and np.all(val[lo_] == np.exp(-200.0)), (name, route)
            un = mx.units(val, ref, scale)
            worst.add(route, "density", un, name, c)
    worst.report("clip")
    for (route, q), (v, where) in worst.w.items():
        assert v <= mc.device_tolerance(mc.cases()[where], "density"), (route, where, v)


def _integrals(case, lam, lo, hi, degree):
    from mlmc_amd.tool import simple_distribution as sd
    return sd._device_integrals(_fn(case), lam, case.sigma, lo, hi, degree)


def test_density_integrate_against_the_reference(hip, converged):
    """mlmc_density_integrate for degree 1, 2, 10, 21, 64 on 257 intervals (the whole domain, a zero-width interval, reversed
    limits, two cdf partitions), on prefixes of 1, 256 and 257 intervals, at converged and perturbed multipliers of every case;
    degree 0 and 65 raise."""
    worst, failures = Worst(), []
    for c in mc.cases().values():
        lo, hi = mc.integrate_intervals(c.domain)
        assert lo[1] == hi[1] and lo[2] > hi[2]
        for tag, lam in (("converged", converged[c.name]), ("perturbed", mc.perturbed(converged[c.name]))):
            for deg in mc.INTEGRATE_DEGREES:
                ref, scale = mx.integrate_ld(c.desc, lam, c.sigma, lo, hi, deg)
                rev, _ = mx.integrate_ld(c.desc, lam, c.sigma, hi[2:3], lo[2:3], deg)
                assert ref[1] == 0 and abs(ref[2] + rev[0]) <= 2.0 ** -60 * scale[2]       # what the reference formula gives
                for n in (1, 256, 257):
                    got = _integrals(c, lam, lo[:n], hi[:n], deg)
                    if n > 1 and not got[1] == 0.0:
                        failures.append(f"{c.name} {tag} degree {deg}: zero-width interval gives {got[1]!r}")
                    un = mx.units(got, ref[:n], scale[:n])
                    worst.add(f"degree {deg}", "integral", un, f"{c.name} {tag} n={n}", c)
                    if not un <= mc.device_tolerance(c, "integral"):
                        failures.append(f"{c.name} {tag} degree {deg} n={n}: {un:.4g} units off (tolerance {mc.device_tolerance(c, 'integral'):g})")
        for deg in (0, 65):
            with pytest.raises(hip.MlmcHipError, match="degree"):
                _integrals(c, converged[c.name], lo[:4], hi[:4], deg)
    worst.report("integrate")
    print("\n".join(failures))
    assert not failures, f"{len(failures)} findings, first: {failures[0]}"


def _check_cdf(case, lam, sigma, got, values, worst, tag):
    lo, hi = mc.cdf_partition(case.domain, values)
    ref, scale = mx.integrate_ld(case.desc, lam, sigma, lo, hi, 10)
    want, k, last = np.empty(len(values), dtype=LD), 0, LD(0)
    bound, acc, added = np.zeros(len(values), dtype=LD), LD(0), 0
    for i, v in enumerate(values):
        if v <= case.domain[0]:
            last, acc, added = LD(0), LD(0), 0
        elif v >= case.domain[1]:
            last, acc, added = LD(1), LD(0), 0
        else:
            last, acc, added = last + ref[k], acc + scale[k], added + 1
            k += 1
        # every piece within the integral tolerance of its scale, plus one rounding of the running fp64 sum per piece added
        want[i], bound[i] = last, mc.device_tolerance(case, "integral") * acc + added * abs(last)
    un = mx.units(got, want, bound + 1e-300)
    worst.add("cdf", "cdf", un, tag, case)
    assert un <= 1.0, (tag, un)


def test_cdf_against_the_reference(hip):
    """SimpleDistribution.cdf and Distribution.cdf on the G6 grids against the prefix sum of the reference's interval integrals
    (the rtol 1e-5 fixture checks of the other modules stay as they are)."""
    from mlmc_amd import Legendre
    from mlmc_amd.tool import distribution as dd
    from mlmc_amd.tool import simple_distribution as sd
    g6 = np.load(os.path.join(mc.GOLDEN, "G6_maxent.npz"))
    worst = Worst()
    for key in mc.G6_KEYS:
        c = mc.cases()[key]
        d = sd.SimpleDistribution(_fn(c), g6[key + "_moment_data"].copy(), domain=c.domain)
        assert d.estimate_density_minimize(tol=1e-8).success
        for values in (g6[key + "_xgrid"][::8], g6[key + "_xgrid"]):
            _check_cdf(c, d.multipliers, d._moment_errs, d.cdf(values), values, worst, key)
    for name in ("norm12", "norm110", "lognorm"):
        for R in (5, 11):
            key = f"{name}_old_R{R}"
            dom = tuple(float(v) for v in g6[key + "_domain"])
            desc = mx.Desc(mx.LEGENDRE, R, dom)
            c = mc.Case(key, desc, np.zeros(R), np.ones(R), np.zeros(R), "g6")
            d = dd.Distribution(Legendre(R, dom), g6[key + "_moment_data"].copy(), domain=dom, force_decay=(True, True))
            assert d.estimate_density_minimize(tol=1e-6, reg_param=0.0).success
            values = g6[key + "_xgrid"]
            _check_cdf(c, d.multipliers, d._moment_errs, d.cdf(values), values, worst, key)
    worst.report("cdf (units of its own bound)")
