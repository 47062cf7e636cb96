"""GPU tests of the batched CDFs and quantiles of the max-entropy densities (mlmc_amd/csrc/density.hip) through the public
entries: simple_distribution.quantiles / cdfs_on_rule / cdfs, SimpleDistribution.quantile, Distribution.quantile,
Estimate.estimate_component_quantiles and the three C entries.

The function that is inverted, Fhat (include/mlmc_hip.h), is a finite sum; tests/quantile_cases.py evaluates it in 80-bit long
double.  For every returned x = Q(p) the main test requires
    |Fhat_ref(x) - p| <= tol_units 2^-53 (scale(x) + p) + 4 rho_ref(x) spacing(x) / T,
tol_units = 4 x the worst error of the fp64 twin on the CPU (qc.TWIN_UNITS_Q, tests/test_quantile_cpu.py), at least 16.  The
worst units per tolerance class are printed before the assertion (pytest -s)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import maxent_cases as mc
from tests import maxent_exact as mx
from tests import quantile_cases as qc

pytestmark = pytest.mark.gpu
LD = np.longdouble
U = 2.0 ** -53


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
    return _FNS[case.name]


def _dist(case, lam, quad, cls=None):
    """a distribution object holding the given multipliers on the given rule"""
    from mlmc_amd.tool import simple_distribution as sd
    cls = sd.SimpleDistribution if cls is None else cls
    d = cls(_fn(case), np.stack([case.mu, case.sigma ** 2], axis=1), domain=case.domain)
    d.multipliers = np.array(lam, dtype=np.float64)
    d._moment_errs = case.sigma.copy()
    d.n_intervals, d._gauss_degree = quad
    return d


@pytest.fixture(scope="module")
def table(hip):
    """the problems: every case on both rules at the multipliers the device solver returns at tol = 1e-8 and at the perturbed
    ones; the unresolved perturbed problems are left out by the reference alone (at most the four named ones)"""
    from mlmc_amd.tool import simple_distribution as sd

    def converged(case, quad):
        lam, _, _, info = sd._solve_on_device(_fn(case), case.mu, case.sigma, case.domain, case.lam0, 1e-8, 100,
                                              n_intervals=quad[0], gauss_degree=quad[1])
        assert info.success == 1, (case.name, quad)
        return lam
    probs = qc.problems(converged)
    used = qc.used_problems(probs)
    out = []
    for case, kind, lam, quad in used:
        out.append(dict(case=case, kind=kind, lam=lam, quad=quad, ref=qc.RuleTable(case, lam, quad), dist=_dist(case, lam, quad),
                        tag=f"{case.name} {kind} {quad[0]}x{quad[1]}"))
    return probs, out


def _by_rule(problems):
    return [[p for p in problems if p["quad"] == quad] for quad in qc.RULES]


def _quantile_failures(problems, p, xs, title):
    worst, failures = {}, []
    for pr, x in zip(problems, xs):
        u = qc.quantile_units(pr["ref"], p, x)
        k = int(np.argmax(u))
        cls = mc.tolerance_class(pr["case"])
        if u[k] > worst.get(cls, (-1.0, None))[0]:
            worst[cls] = (float(u[k]), f"{pr['tag']} p = {p[k]:.6g}")
        if not u[k] <= qc.quantile_tolerance(pr["case"]):
            failures.append(f"{pr['tag']}: {u[k]:.4g} units at p = {p[k]:.6g} (tolerance {qc.quantile_tolerance(pr['case']):g})")
    print()
    for cls, (v, where) in sorted(worst.items()):
        print(f"{title}: worst {cls:8s} {v:10.4g} units at {where}")
    return failures


def test_left_out_problems(table):
    probs, used = table
    assert len(probs) == 4 * len(mc.cases())
    left = [(c.name, k, q) for c, k, l, q, r in probs if r > qc.RESOLVED_RTOL]
    print("\nleft out:", left)
    assert all(k == "perturbed" and n in qc.MAY_BE_UNRESOLVED for n, k, q in left)
    assert len(used) == len(probs) - len(left) and len(left) <= 2 * len(qc.MAY_BE_UNRESOLVED)


def test_quantiles_accuracy(hip, table):
    """every x = Q(p), 0 < p < 1, of every used problem against the long-double Fhat"""
    from mlmc_amd.tool import simple_distribution as sd
    failures = []
    for group in _by_rule(table[1]):
        xs = sd.quantiles([p["dist"] for p in group], qc.GRID)
        assert len(xs) == len(group) and all(x.shape == qc.GRID.shape for x in xs)
        for pr, x in zip(group, xs):
            assert np.all((x >= pr["case"].domain[0]) & (x <= pr["case"].domain[1])), pr["tag"]
        failures += _quantile_failures(group, qc.GRID, xs, f"quantiles {group[0]['quad'][0]}x{group[0]['quad'][1]}")
    assert not failures, "\n".join(failures)


def test_specials(hip, table):
    from mlmc_amd.tool import simple_distribution as sd
    for group in _by_rule(table[1]):
        batch = sd.quantiles([p["dist"] for p in group], qc.SPECIALS)
        for pr, x in zip(group, batch):
            a, b = pr["case"].domain
            assert x[0] == a and x[1] == b and x[2] == a, pr["tag"]
            assert np.all(np.isnan(x[3:])), pr["tag"]
            single = pr["dist"].quantile(qc.SPECIALS)
            assert np.array_equal(np.isnan(single), np.isnan(x)) and np.array_equal(single, x, equal_nan=True), pr["tag"]


def test_monotone(hip, table):
    from mlmc_amd.tool import simple_distribution as sd
    grid = np.sort(np.concatenate([qc.GRID, [0.0, 1.0]]))
    inner = (grid >= 0.001) & (grid <= 0.999)
    for group in _by_rule(table[1]):
        for pr, x in zip(group, sd.quantiles([p["dist"] for p in group], grid)):
            assert np.all(np.diff(x) >= 0), pr["tag"]
            assert np.all(np.diff(x[inner]) > 0), pr["tag"]


def test_uniform_closed_form(hip):
    """R1 = 1, lambda_0 = log(b - a): Q(p) = a + p (b - a) within 16 spacings of max(|a|, |b|)"""
    import mlmc_amd
    from mlmc_amd.tool import simple_distribution as sd
    p = qc.GRID
    for dom in ((-4.0, 6.0), (0.2, 12.0), (1e3, 1e3 + 1e-2)):
        a, b = dom
        d = sd.SimpleDistribution(mlmc_amd.Legendre(1, dom), np.array([[1.0, 1.0]]), domain=dom)
        d.multipliers, d._moment_errs = np.array([np.log(b - a)]), np.ones(1)
        x = d.quantile(p)
        err = np.abs(x.astype(LD) - (LD(a) + p.astype(LD) * (LD(b) - LD(a))))
        sp = np.spacing(max(abs(a), abs(b)))
        print(f"\nuniform {dom}: worst {float(np.max(err)) / sp:.3g} spacings")
        assert np.all(err <= 16 * sp), (dom, float(np.max(err)) / sp)


def test_gaussian_closed_form(hip):
    """Legendre R1 = 3 on [-8, 8], lambda = (32/3 + log(2 pi) / 2, 0, 64/3): the standard normal density"""
    import mlmc_amd
    from scipy.stats import norm
    from mlmc_amd.tool import simple_distribution as sd
    dom = (-8.0, 8.0)
    d = sd.SimpleDistribution(mlmc_amd.Legendre(3, dom), np.stack([np.eye(3)[0], np.ones(3)], axis=1), domain=dom)
    d.multipliers, d._moment_errs = np.array([32.0 / 3 + 0.5 * np.log(2 * np.pi), 0.0, 64.0 / 3]), np.ones(3)
    p = np.concatenate([[1e-6, 1e-4], qc.GRID_INNER, [1 - 1e-4, 1 - 1e-6]])
    x = d.quantile(p)
    err = np.abs(norm.cdf(x) - p)
    print(f"\ngaussian: worst |Phi(Q(p)) - p| = {np.max(err):.3g}")
    assert np.all(err <= 1e-14), np.max(err)


def test_cdfs_on_rule_and_round_trip(hip, table):
    """Fhat on the device against the reference at the density points in units of scale(x); cdfs_on_rule(quantiles(p)) against p
    under the bound of the accuracy test; mass_out against the long-double T"""
    from mlmc_amd.tool import simple_distribution as sd
    failures, worst = [], {}

    def note(key, case, value, where):
        key = f"{key}/{mc.tolerance_class(case)}"
        if value > worst.get(key, (-1.0, None))[0]:
            worst[key] = (value, where)
    for group in _by_rule(table[1]):
        distrs = [p["dist"] for p in group]
        pts = [mc.density_points(p["case"].domain) for p in group]
        got, mass = sd._on_rule(distrs, pts, False, "cdfs_on_rule")
        assert all(np.array_equal(g, h, equal_nan=True) for g, h in zip(got, sd.cdfs_on_rule(distrs, pts)))
        xs = sd.quantiles(distrs, qc.GRID)
        back = sd.cdfs_on_rule(distrs, xs)
        for pr, x, f, m, q, fb in zip(group, pts, got, mass, xs, back):
            case, ref = pr["case"], pr["ref"]
            tol = mc.device_tolerance(case, "integral")
            F, sc = ref.fhat(x)
            un = mx.units(f, F, sc)
            note("Fhat", case, un, pr["tag"])
            if not un <= tol:
                failures.append(f"{pr['tag']}: Fhat is {un:.4g} units off (tolerance {tol:g})")
            un = mx.units(m, ref.T, ref.S[-1])
            note("mass", case, un, pr["tag"])
            if not un <= tol:
                failures.append(f"{pr['tag']}: mass is {un:.4g} units off (tolerance {tol:g})")
            _, sq = ref.fhat(q)
            slack = 4 * ref.density(q) * np.spacing(np.abs(q)).astype(LD) / ref.T
            err = np.maximum(np.abs(fb.astype(LD) - qc.GRID.astype(LD)) - slack, 0) / (LD(U) * (sq + qc.GRID.astype(LD)))
            un = float(np.max(err))
            note("round trip", case, un, pr["tag"])
            if not un <= qc.quantile_tolerance(case):
                failures.append(f"{pr['tag']}: round trip is {un:.4g} units off (tolerance {qc.quantile_tolerance(case):g})")
    print()
    for key, (v, where) in sorted(worst.items()):
        print(f"worst {key:20s} {v:10.4g} units at {where}")
    assert not failures, "\n".join(failures)


def test_cdfs_bit_for_bit(hip, table):
    """cdfs == [d.cdf(v)] on the G6 grids for SimpleDistribution and Distribution, with values outside the domain and unsorted
    values; one array for all distributions as well"""
    from mlmc_amd.tool import simple_distribution as sd
    from mlmc_amd.tool.distribution import Distribution
    g6 = np.load(os.path.join(mc.GOLDEN, "G6_maxent.npz"))
    rng = np.random.default_rng(5)
    group = [p for p in table[1] if p["case"].name in mc.G6_KEYS and p["quad"] == (64, 21) and p["kind"] == "converged"]
    assert len(group) == len(mc.G6_KEYS)
    for cls in (sd.SimpleDistribution, Distribution):
        distrs = [_dist(p["case"], p["lam"], p["quad"], cls) for p in group]
        grids = []
        for p in group:
            xg = np.array(g6[p["case"].name + "_xgrid"], dtype=np.float64)
            a, b = p["case"].domain
            grids.append(np.concatenate([[a - 1.0, a], xg[::8], [b, b + 2.0], rng.permutation(xg[::16]), [np.nextafter(a, b)]]))
        want = [d.cdf(v) for d, v in zip(distrs, grids)]
        got = sd.cdfs(distrs, grids)
        for p, g, w in zip(group, got, want):
            assert g.shape == w.shape and np.array_equal(g, w, equal_nan=True), (cls.__name__, p["tag"])
        common = np.linspace(-3.0, 3.0, 77)
        for d, g in zip(distrs, sd.cdfs(distrs, common)):
            assert np.array_equal(g, d.cdf(common), equal_nan=True)


def _raw_args(hip, problems):
    B = len(problems)
    r1 = np.array([len(p["lam"]) for p in problems], dtype=np.int32)
    ldv = int(r1.max())
    lam, sig = np.zeros((B, ldv)), np.ones((B, ldv))
    for i, p in enumerate(problems):
        lam[i, :r1[i]], sig[i, :r1[i]] = p["lam"], p["case"].sigma[:r1[i]]
    handles = (C.c_void_p * B)(*[_fn(p["case"])._basis_handle().value for p in problems])
    return handles, r1, lam, sig


def test_integrate_batch_bit_for_bit(hip, table):
    """mlmc_density_integrate_batch == mlmc_density_integrate per problem on mc.integrate_intervals, every degree, a problem
    without intervals in the middle of the batch"""
    from mlmc_amd.tool import simple_distribution as sd
    names = ("norm12_R21", "mix_R26", "monomial_R6", "fourier_R9", "spline_R10", "log_legendre_R8", "partial_R9_of_norm12_R21", "shifted_R6")
    group = [p for p in table[1] if p["case"].name in names and p["quad"] == (64, 21)]
    assert len(group) == 2 * len(names)
    handles, r1, lam, sig = _raw_args(hip, group)
    empty = len(group) // 2
    ivs = [mc.integrate_intervals(p["case"].domain) for p in group]
    ivs[empty] = (np.zeros(0), np.zeros(0))
    lo = np.ascontiguousarray(np.concatenate([iv[0] for iv in ivs]))
    hi = np.ascontiguousarray(np.concatenate([iv[1] for iv in ivs]))
    n = np.array([len(iv[0]) for iv in ivs], dtype=np.int64)
    for deg in mc.INTEGRATE_DEGREES:
        out = np.full(lo.shape, 7.25)
        hip.check(hip.lib().mlmc_density_integrate_batch(len(group), C.cast(handles, C.c_void_p), hip.ptr(r1), hip.ptr(lam), hip.ptr(sig),
                                                         hip.ptr(lo), hip.ptr(hi), hip.ptr(n), deg, hip.ptr(out)))
        off = 0
        for p, iv in zip(group, ivs):
            if len(iv[0]):
                want = sd._device_integrals(_fn(p["case"]), p["lam"], p["case"].sigma, iv[0], iv[1], deg)
                assert np.array_equal(out[off:off + len(iv[0])], want, equal_nan=True), (p["tag"], deg)
            off += len(iv[0])


def test_batch_independence(hip, table):
    """a problem alone == in a shuffled batch of all problems; 1500 copies of one problem all identical; a probability alone ==
    inside an array of 10^6; host p == device p"""
    import torch
    from mlmc_amd.tool import simple_distribution as sd
    rng = np.random.default_rng(9)
    p_all = np.concatenate([qc.GRID, qc.SPECIALS])
    for group in _by_rule(table[1]):
        distrs = [p["dist"] for p in group]
        alone = [d.quantile(p_all) for d in distrs]
        alone_f = [sd.cdfs_on_rule([d], a)[0] for d, a in zip(distrs, alone)]
        perm = rng.permutation(len(group))
        shuffled = sd.quantiles([distrs[i] for i in perm], p_all)
        shuffled_f = sd.cdfs_on_rule([distrs[i] for i in perm], [alone[i] for i in perm])
        for k, i in enumerate(perm):
            assert np.array_equal(shuffled[k], alone[i], equal_nan=True), group[i]["tag"]
            assert np.array_equal(shuffled_f[k], alone_f[i], equal_nan=True), group[i]["tag"]
    pr = [p for p in table[1] if p["case"].name == "norm12_R21" and p["kind"] == "converged" and p["quad"] == (64, 21)][0]
    d = pr["dist"]
    B = 1500
    assert B > hip.device_info()["n_cu"]
    probs3 = np.array([0.05, 0.5, 0.95])
    copies = sd.quantiles([d] * B, probs3)
    want = d.quantile(probs3)
    assert len(copies) == B and all(np.array_equal(c, want) for c in copies)
    # one probability alone and inside 10^6 others; host and device probabilities
    many = rng.random(1_000_000)
    many[123_457] = 0.3125
    got = d.quantile(many)
    assert got[123_457] == d.quantile(0.3125)[0]
    dev = d.quantile(torch.from_numpy(many).cuda())
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.shape == (1_000_000,)
    assert np.array_equal(dev.cpu().numpy(), got)
    assert np.all(np.diff(got[np.argsort(many)]) >= 0)
    from mlmc_amd.tool.distribution import Distribution
    old = _dist(pr["case"], pr["lam"], pr["quad"], Distribution)
    assert np.array_equal(old.quantile(probs3), want)


def test_two_runs_give_the_same_bits(hip, table):
    from mlmc_amd.tool import simple_distribution as sd
    p_all = np.concatenate([qc.GRID, qc.SPECIALS])
    for group in _by_rule(table[1]):
        distrs = [p["dist"] for p in group]
        q1, q2 = sd.quantiles(distrs, p_all), sd.quantiles(distrs, p_all)
        f1, f2 = sd.cdfs_on_rule(distrs, q1), sd.cdfs_on_rule(distrs, q1)
        finite = [q[np.isfinite(q)] for q in q1]             # cdf(), and hence cdfs(), has no defined result for NaN values
        c1, c2 = sd.cdfs(distrs, finite), sd.cdfs(distrs, finite)
        for a, b in zip(q1 + f1 + c1, q2 + f2 + c2):
            assert np.array_equal(a, b, equal_nan=True)


def test_argument_errors(hip, table):
    from mlmc_amd import Legendre
    from mlmc_amd.tool import simple_distribution as sd
    lib = hip.lib()
    dom = (-2.0, 2.0)
    B = 4
    fns = [Legendre(5, dom) for _ in range(B)]
    handles = (C.c_void_p * B)(*[f._basis_handle().value for f in fns])
    hp = C.cast(handles, C.c_void_p)
    r1 = np.full(B, 5, dtype=np.int32)
    lam, sig = np.zeros((B, 5)), np.ones((B, 5))
    lam[:, 0] = np.log(4.0)
    a, b = np.full(B, dom[0]), np.full(B, dom[1])
    p = np.full(2 * B, 0.5)
    n = np.full(B, 2, dtype=np.int64)
    out, mass = np.empty(2 * B), np.empty(B)
    P = hip.ptr

    def on_rule(fn, **kw):
        v = dict(B=B, h=hp, r1=r1, lam=lam, sig=sig, a=a, b=b, ni=0, deg=0, p=p, n=n, out=out, mass=mass, kind=hip.HOST)
        v.update(kw)
        return fn(v["B"], v["h"], P(v["r1"]), P(v["lam"]), P(v["sig"]), P(v["a"]), P(v["b"]), v["ni"], v["deg"], P(v["p"]), P(v["n"]),
                  P(v["out"]), P(v["mass"]), v["kind"])

    def integ(**kw):
        v = dict(B=B, h=hp, r1=r1, lam=lam, sig=sig, lo=p, hi=p, n=n, deg=10, out=out)
        v.update(kw)
        return lib.mlmc_density_integrate_batch(v["B"], v["h"], P(v["r1"]), P(v["lam"]), P(v["sig"]), P(v["lo"]), P(v["hi"]), P(v["n"]),
                                                v["deg"], P(v["out"]))

    def expect(rc, pattern):
        with pytest.raises(hip.MlmcHipError, match=pattern):
            hip.check(rc)
    bad_r1 = r1.copy(); bad_r1[2] = 6
    bad_n = n.copy(); bad_n[1] = -1
    bad_b = b.copy(); bad_b[3] = dom[0]
    inf_a = a.copy(); inf_a[1] = -np.inf
    nan_b = b.copy(); nan_b[0] = np.nan
    null_h = (C.c_void_p * B)(*[f._basis_handle().value for f in fns])
    null_h[2] = None
    for fn, name in ((lib.mlmc_density_cdf_batch, "mlmc_density_cdf_batch"), (lib.mlmc_density_quantiles_batch, "mlmc_density_quantiles_batch")):
        assert on_rule(fn) == 0
        expect(on_rule(fn, r1=bad_r1), name + ": problem 2.*R1")
        expect(on_rule(fn, n=bad_n), name + ": problem 1.*n < 0")
        expect(on_rule(fn, b=bad_b), name + ": problem 3.*domain")
        expect(on_rule(fn, a=inf_a), name + ": problem 1.*domain")
        expect(on_rule(fn, b=nan_b), name + ": problem 0.*domain")
        expect(on_rule(fn, h=C.cast(null_h, C.c_void_p)), name + ": problem 2.*null basis")
        expect(on_rule(fn, deg=65), name + ".*gauss_degree")
        expect(on_rule(fn, deg=-1), name + ".*gauss_degree")
        expect(on_rule(fn, ni=-1), name + ".*n_intervals")
        expect(on_rule(fn, B=-1), name + ".*B < 0")
        expect(fn(B, hp, P(r1), P(lam), P(sig), None, P(b), 0, 0, P(p), P(n), P(out), P(mass), hip.HOST), name + ".*null")
        expect(fn(B, hp, P(r1), P(lam), P(sig), P(a), P(b), 0, 0, None, P(n), P(out), P(mass), hip.HOST), name + ".*null")
        assert fn(0, None, None, None, None, None, None, 0, 0, None, None, None, None, hip.HOST) == 0
        # no points at all: a no-op that still reports the masses; NULL mass_out is accepted
        mass[:] = -1.0
        assert on_rule(fn, n=np.zeros(B, dtype=np.int64), p=None, out=None) == 0 and np.all(np.abs(mass - 1.0) < 1e-12)
        assert fn(B, hp, P(r1), P(lam), P(sig), P(a), P(b), 0, 0, P(p), P(n), P(out), None, hip.HOST) == 0
    # an IDENTITY basis (a plain quantity: no moments, no density) at a known index
    from mlmc_amd.engine import _IdentityBasis
    ident = _IdentityBasis()
    id_h = (C.c_void_p * B)(*[f._basis_handle().value for f in fns])
    id_h[1] = ident._basis_handle().value
    id_r1 = r1.copy(); id_r1[1] = 1
    for fn, name in ((lib.mlmc_density_cdf_batch, "mlmc_density_cdf_batch"), (lib.mlmc_density_quantiles_batch, "mlmc_density_quantiles_batch")):
        expect(on_rule(fn, h=C.cast(id_h, C.c_void_p), r1=id_r1), name + ": problem 1.*unsupported basis kind")
    expect(integ(h=C.cast(id_h, C.c_void_p), r1=id_r1), "mlmc_density_integrate_batch: problem 1.*unsupported basis kind")
    # a [B, n] array is ambiguous in the Python layer
    with pytest.raises(ValueError, match="ambiguous"):
        sd.quantiles([p["dist"] for p in table[1][:2]], np.full((2, 3), 0.5))
    assert integ() == 0
    expect(integ(r1=bad_r1), "mlmc_density_integrate_batch: problem 2.*R1")
    expect(integ(n=bad_n), "mlmc_density_integrate_batch: problem 1.*n < 0")
    expect(integ(h=C.cast(null_h, C.c_void_p)), "mlmc_density_integrate_batch: problem 2.*null basis")
    expect(integ(deg=0), "mlmc_density_integrate_batch.*degree")
    expect(integ(deg=65), "mlmc_density_integrate_batch.*degree")
    expect(integ(lo=None), "mlmc_density_integrate_batch.*null")
    assert lib.mlmc_density_integrate_batch(0, None, None, None, None, None, None, None, 10, None) == 0
    # a problem whose mass is not finite and positive: NaN for all its points, no error
    over = lam.copy()
    over[1, 0] = -1e6                                  # exponent clipped at +200 everywhere: the mass 4 e^200 is finite ...
    wide_a = a.copy()
    wide_a[2] = -3.0                                   # ... cells outside the domain of the moments: the density is NaN there
    for fn in (lib.mlmc_density_cdf_batch, lib.mlmc_density_quantiles_batch):
        out[:] = 7.25
        assert on_rule(fn, lam=over, a=wide_a) == 0
        assert np.all(np.isnan(out[4:6])) and np.isnan(mass[2]) and not np.any(np.isnan(np.delete(out, [4, 5])))
        assert abs(mass[1] / (4 * np.exp(200.0)) - 1) < 1e-12
    # the Python layer: mixed rules
    group = [p for p in table[1] if p["kind"] == "converged" and p["case"].name == "mix_R9"]
    assert len(group) == 2
    with pytest.raises(ValueError, match="same quadrature"):
        sd.quantiles([p["dist"] for p in group], [0.5])
    with pytest.raises(ValueError, match="same quadrature"):
        sd.cdfs_on_rule([p["dist"] for p in group], [0.5])


# ---- Estimate.estimate_component_quantiles --------------------------------------------------------------------------------
def _device_vector_storage():
    import torch
    from tests.util import level_arrays
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    from mlmc_amd.sample_storage import DeviceMemory
    M, steps = 12, [0.5, 0.07, 0.01]
    levels = level_arrays([20000, 4000, 1200], steps, M, 0, seed=77)
    spec = [QuantitySpec(name="q", unit="m", shape=(4, 1), times=[1, 2, 3], locations=['0'])]
    dev = DeviceMemory()
    dev.save_global_data(result_format=spec, level_parameters=[[s] for s in steps])
    for l, (f, c) in enumerate(levels):
        f = f.copy()
        c = np.zeros_like(f) if c is None else c.copy()
        for m in range(M):
            for arr in (f, c):
                arr[m] = 0.1 * (m % 5 - 2) + (0.7 + 0.05 * m) * (arr[m] - 0.125 * m)
        f[1, 7::53] = np.nan
        f[3, 11::41] = np.nan
        if l > 0:
            c[2, 5::37] = np.nan
        dev.set_level_samples(l, torch.from_numpy(np.stack([f, c], axis=-1)).cuda())
    return dev, spec, M


def test_estimate_component_quantiles(hip):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate, scalar_component
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.tool import simple_distribution as sd
    dev, spec, M = _device_vector_storage()
    qe.device_cache_clear()
    q = make_root_quantity(dev, spec)['q']
    doms = Estimate.estimate_domains(q, dev)
    fns = [Legendre(11, tuple(doms[m])) for m in range(M)]
    est = Estimate(q, dev, fns[0])
    probs = np.concatenate([[0.001, 0.05, 0.5, 0.95, 0.999], np.linspace(0.01, 0.99, 99)])
    quant, success = est.estimate_component_quantiles(probs, tol=1e-8, orth_moments_tol=1e-4, moments_fns=fns)
    assert quant.shape == (M, probs.size) and success.shape == (M,) and success.dtype == bool
    dens = est.construct_densities(tol=1e-8, orth_moments_tol=1e-4, moments_fns=fns)
    want = sd.quantiles([d[0] for d in dens], probs)
    assert np.array_equal(quant, np.array(want))
    assert np.array_equal(success, np.array([bool(d[2].success) for d in dens])) and success.all()
    again, success2 = est.estimate_component_quantiles(probs, densities=dens)
    assert np.array_equal(again, quant) and np.array_equal(success2, success)
    worst = 0.0
    for m in range(M):
        d_m = Estimate(scalar_component(q, m), dev, fns[m]).construct_density(tol=1e-8, orth_moments_tol=1e-4)[0]
        err = np.abs(sd.cdfs_on_rule([d_m], quant[m])[0] - probs)
        worst = max(worst, float(np.max(err)))
        assert np.all(err <= 2e-5), (m, float(np.max(err)))
    print(f"\ncomponent quantiles against the scalar chain: worst |Fhat_m(q) - p| = {worst:.3g}")
