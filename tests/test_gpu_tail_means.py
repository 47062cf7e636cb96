"""GPU tests of the batched tail means (expected shortfall) of the max-entropy densities (k_q_cells<true>, k_q_prefix<true>, k_q_tails
in mlmc_amd/csrc/density.hip) through the public entries: simple_distribution.tail_means, SimpleDistribution / Distribution
.expected_shortfall, Estimate.estimate_component_shortfall / bootstrap_component_shortfall and mlmc_density_tail_means_batch.

lower(x) and upper(x) (include/mlmc_hip.h) are finite sums; tests/tail_cases.py evaluates them in 80-bit long double AT THE
QUANTILES THE DEVICE RETURNED.  The main test requires |value - reference| <= tol_units 2^-53 scale, tol_units = 4 x the worst
error of the fp64 twin on the CPU (tc.TWIN_UNITS_T, tests/test_tail_means_cpu.py), at least 16.  The worst units per tolerance
class are printed before the assertion (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

from tests import maxent_cases as mc
from tests import quantile_cases as qc
from tests import tail_cases as tc
from tests.test_gpu_quantiles import _dist, _fn

pytestmark = pytest.mark.gpu
LD = np.longdouble
U = 2.0 ** -53
P_ALL = np.concatenate([tc.GRID, qc.SPECIALS])


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


@pytest.fixture(scope="module")
def table(hip):
    """every used problem (qc.used_problems: converged multipliers of the device solver and the perturbed ones, both rules) with its
    long-double table, and ONE tail_means call per rule over tc.GRID and the special probabilities, shared by the tests"""
    from mlmc_amd.tool import simple_distribution as sd

    def converged(case, quad):
        lam, _, _, info = sd._solve_on_device(_fn(case), case.mu, case.sigma, case.domain, case.lam0, 1e-8, 100,
                                              n_intervals=quad[0], gauss_degree=quad[1])
        assert info.success == 1, (case.name, quad)
        return lam
    probs = qc.problems(converged)
    out = []
    for case, kind, lam, quad in qc.used_problems(probs):
        out.append(dict(case=case, kind=kind, lam=lam, quad=quad, ref=tc.TailTable(case, lam, quad), dist=_dist(case, lam, quad),
                        tag=f"{case.name} {kind} {quad[0]}x{quad[1]}"))
    for quad in qc.RULES:
        group = [p for p in out if p["quad"] == quad]
        (q, lower, upper, mean), mass = sd._on_rule([p["dist"] for p in group], [P_ALL] * len(group), True, "tail_means", tails=True)
        for k, pr in enumerate(group):
            pr.update(q=q[k], lower=lower[k], upper=upper[k], mean=mean[k], mass=mass[k], ref_tails=pr["ref"].tails(q[k][:tc.GRID.size]))
    return probs, out


def _by_rule(problems):
    return [[p for p in problems if p["quad"] == quad] for quad in qc.RULES]


def test_used_problems(table):
    probs, used = table
    left = [(c.name, k, q) for c, k, l, q, r in probs if r > qc.RESOLVED_RTOL]
    print("\nleft out:", left)
    assert len(probs) == 4 * len(mc.cases()) and len(used) == len(probs) - len(left)
    assert all(k == "perturbed" and n in qc.MAY_BE_UNRESOLVED for n, k, q in left) and len(left) <= 2 * len(qc.MAY_BE_UNRESOLVED)
    assert all(len(g) <= 2 * len(mc.cases()) for g in _by_rule(used))


def test_accuracy(hip, table):
    """q bit for bit the quantile entry's, lower / upper against the long-double tails at q, the mass bit for bit the quantile
    entry's, the mean against a + V_n / T"""
    from mlmc_amd.tool import simple_distribution as sd
    failures, worst = [], {}

    def note(key, case, value, where):
        key = f"{key}/{mc.tolerance_class(case)}"
        if value > worst.get(key, (-1.0, None))[0]:
            worst[key] = (value, where)
    n = tc.GRID.size
    for group in _by_rule(table[1]):
        distrs = [p["dist"] for p in group]
        want_q, want_mass = sd._on_rule(distrs, [P_ALL] * len(group), True, "quantiles")
        for pr, wq, wm in zip(group, want_q, want_mass):
            case, tol = pr["case"], tc.tail_tolerance(pr["case"])
            assert pr["q"].shape == P_ALL.shape and np.array_equal(pr["q"], wq, equal_nan=True), pr["tag"]
            assert pr["mass"] == wm, pr["tag"]
            rl, ru, sl, su = pr["ref_tails"]
            for name, got, want, sc in (("lower", pr["lower"][:n], rl, sl), ("upper", pr["upper"][:n], ru, su)):
                assert np.all(np.isfinite(got)), (pr["tag"], name)
                u = (np.abs(got.astype(LD) - want) / (LD(U) * sc)).astype(np.float64)
                k = int(np.argmax(u))
                note(name, case, float(u[k]), f"{pr['tag']} p = {tc.GRID[k]:.6g}")
                if not u[k] <= tol:
                    failures.append(f"{pr['tag']}: {name} is {u[k]:.4g} units off at p = {tc.GRID[k]:.6g} (tolerance {tol:g})")
            m, sm = pr["ref"].mean()
            u = float(abs(LD(pr["mean"]) - m) / (LD(U) * sm))
            note("mean", case, u, pr["tag"])
            if not u <= tol:
                failures.append(f"{pr['tag']}: mean is {u:.4g} units off (tolerance {tol:g})")
    print()
    for key, (v, where) in sorted(worst.items()):
        print(f"worst {key:16s} {v:10.4g} units at {where}")
    assert not failures, "\n".join(failures)


def test_specials(hip, table):
    """p = 0, 1, -0.0 give (a, a, upper(a)) and (b, lower(b), b); NaN, -0.1, 1.1, +-inf give NaN in all three outputs; a problem
    whose mass is not finite gives NaN everywhere and no error"""
    from mlmc_amd.tool import simple_distribution as sd
    n = tc.GRID.size
    for pr in table[1]:
        a, b = pr["case"].domain
        q, lower, upper = pr["q"][n:], pr["lower"][n:], pr["upper"][n:]
        tol = tc.tail_tolerance(pr["case"])
        rl, ru, sl, su = pr["ref"].tails([a, b])
        for k in (0, 2):
            assert q[k] == a and lower[k] == a, pr["tag"]
            assert abs(LD(upper[k]) - ru[0]) <= tol * LD(U) * su[0], (pr["tag"], float(abs(LD(upper[k]) - ru[0]) / (LD(U) * su[0])))
        assert q[1] == b and upper[1] == b, pr["tag"]
        assert abs(LD(lower[1]) - rl[1]) <= tol * LD(U) * sl[1], (pr["tag"], float(abs(LD(lower[1]) - rl[1]) / (LD(U) * sl[1])))
        assert np.all(np.isnan(q[3:])) and np.all(np.isnan(lower[3:])) and np.all(np.isnan(upper[3:])), pr["tag"]
    # The exponent is clipped at +-200, so no multipliers make the mass overflow (the mass of the second problem below is
    # 10 e^200); a mass that is not finite comes from a domain that reaches outside the domain of the moments, where the density
    # is NaN
    pr = [p for p in table[1] if p["case"].name == "mix_R9" and p["kind"] == "converged" and p["quad"] == (64, 21)][0]
    case = pr["case"]
    wide = _dist(case, pr["lam"], pr["quad"])
    wide.domain = (case.domain[0] - 1.0, case.domain[1])
    big = pr["lam"].copy()
    big[0] = -1e6
    clipped = _dist(case, big, pr["quad"])
    (q, lower, upper, mean), mass = sd._on_rule([pr["dist"], clipped, wide, pr["dist"]], [P_ALL] * 4, True, "tail_means", tails=True)
    assert np.all(np.isnan(q[2])) and np.all(np.isnan(lower[2])) and np.all(np.isnan(upper[2])) and np.isnan(mass[2]) and np.isnan(mean[2])
    assert abs(mass[1] / (10 * np.exp(200.0)) - 1) < 1e-12 and np.all(np.isfinite(lower[1][:n])) and np.all(np.isfinite(upper[1][:n]))
    for k in (0, 3):
        assert np.array_equal(q[k], pr["q"], equal_nan=True) and np.array_equal(lower[k], pr["lower"], equal_nan=True)
        assert np.array_equal(upper[k], pr["upper"], equal_nan=True) and mean[k] == pr["mean"] and mass[k] == pr["mass"]


def _uniform(dom, log=False):
    import mlmc_amd
    from mlmc_amd.tool import simple_distribution as sd
    a, b = dom
    d = sd.SimpleDistribution(mlmc_amd.Legendre(1, dom, log=log), np.array([[1.0, 1.0]]), domain=dom)
    d.multipliers, d._moment_errs = np.array([np.log(b - a)]), np.ones(1)
    return d


def test_uniform_closed_form(hip):
    """R1 = 1, lambda_0 = log(b - a): lower = (a + Q) / 2, upper = (Q + b) / 2 within 2 (N + 8) 2^-53 (b - a) + 2^-52 max(|a|, |b|),
    N = n_intervals gauss_degree: the recursive-summation bound of the two positive sums of N terms of a quotient, and the
    rounding of the result"""
    from mlmc_amd.tool import simple_distribution as sd
    for dom, log in (((-4.0, 6.0), False), ((0.2, 12.0), True), ((1e3, 1e3 + 1e-2), False)):
        a, b = dom
        d = _uniform(dom, log)
        q, lower, upper, mean = sd.tail_means([d], tc.GRID)
        q, lower, upper = q[0], lower[0], upper[0]
        gate = 2 * (d.n_intervals * d._gauss_degree + 8) * U * (b - a) + 2 * U * max(abs(a), abs(b))
        el = np.abs(lower.astype(LD) - (LD(a) + q.astype(LD)) / 2)
        eu = np.abs(upper.astype(LD) - (q.astype(LD) + LD(b)) / 2)
        em = abs(LD(mean[0]) - (LD(a) + LD(b)) / 2)
        print(f"\nuniform {dom}: worst lower {float(np.max(el)):.3g} upper {float(np.max(eu)):.3g} mean {float(em):.3g} gate {gate:.3g}")
        assert np.all(el <= gate) and np.all(eu <= gate) and em <= gate, (dom, float(np.max(el)), float(np.max(eu)), float(em), gate)
        for tail, want in (("upper", upper), ("lower", lower)):
            assert np.array_equal(d.expected_shortfall(tc.GRID, tail), want)


def _gaussian(mu, sigma, n_intervals=64):
    """Legendre R1 = 3 on (mu - 8 sigma, mu + 8 sigma), lambda = (32/3, 0, 64/3): the exponent is z^2 / 2, z = (x - mu) / sigma"""
    import mlmc_amd
    from mlmc_amd.tool import simple_distribution as sd
    dom = (mu - 8 * sigma, mu + 8 * sigma)
    d = sd.SimpleDistribution(mlmc_amd.Legendre(3, dom), np.stack([np.eye(3)[0], np.ones(3)], axis=1), domain=dom)
    d.multipliers, d._moment_errs = np.array([32.0 / 3, 0.0, 64.0 / 3]), np.ones(3)
    d.n_intervals = n_intervals
    return d


def test_gaussian_closed_form(hip):
    """upper = mu + sigma phi(z_p) / (1 - p), lower = mu - sigma phi(z_p) / p within 32 sigma Phi(-8) / min(p, 1 - p) (the truncation
    of the domain at 8 sigma) + 64 2^-53 (|mu| + 8 sigma) (the rounding of x and of the sums)"""
    from scipy.stats import norm
    from mlmc_amd.tool import simple_distribution as sd
    p = np.array([1e-3, 0.01, 0.05, 0.5, 0.95, 0.99, 0.999])
    z = norm.ppf(p)
    for mu, sigma in ((1.0, 2.0), (1000.0, 0.5)):
        d = _gaussian(mu, sigma)
        q, lower, upper, mean = sd.tail_means([d], p)
        gate = 32 * sigma * norm.cdf(-8.0) / np.minimum(p, 1 - p) + 64 * U * (abs(mu) + 8 * sigma)
        eu = np.abs(upper[0] - (mu + sigma * norm.pdf(z) / (1 - p)))
        el = np.abs(lower[0] - (mu - sigma * norm.pdf(z) / p))
        print(f"\ngaussian ({mu}, {sigma}): worst lower error / gate {np.max(el / gate):.3g}, upper {np.max(eu / gate):.3g}; "
              f"errors in sigma: {np.max(el) / sigma:.3g} {np.max(eu) / sigma:.3g}")
        assert np.all(el <= gate) and np.all(eu <= gate), (mu, sigma, el / gate, eu / gate)
        assert abs(mean[0] - mu) <= gate[3]


def test_order(hip, table):
    """lower <= q <= upper, and both non-decreasing in p over the grid, each up to the unit gate of the accuracy test"""
    n = tc.GRID.size
    for pr in table[1]:
        q, lower, upper = pr["q"][:n].astype(LD), pr["lower"][:n].astype(LD), pr["upper"][:n].astype(LD)
        _, _, sl, su = pr["ref_tails"]
        gl, gu = tc.tail_tolerance(pr["case"]) * LD(U) * sl, tc.tail_tolerance(pr["case"]) * LD(U) * su
        assert np.all(lower - q <= gl) and np.all(q - upper <= gu), pr["tag"]
        assert np.all(np.diff(lower) >= -(gl[1:] + gl[:-1])) and np.all(np.diff(upper) >= -(gu[1:] + gu[:-1])), pr["tag"]
        a, b = pr["case"].domain
        assert np.all((pr["lower"][:n] >= a) & (pr["upper"][:n] <= b)), pr["tag"]


def _same(x, y):
    return all(np.array_equal(u, v, equal_nan=True) for u, v in zip(x, y))


def test_batch_independence_and_two_runs(hip, table):
    """a problem alone == the problem in a shuffled batch of all; one p alone == the p among all; host points == device points;
    two runs give the same bits"""
    import torch
    from mlmc_amd.tool import simple_distribution as sd
    rng = np.random.default_rng(9)
    for group in _by_rule(table[1]):
        distrs = [p["dist"] for p in group]
        perm = rng.permutation(len(group))
        q, lower, upper, mean = sd.tail_means([distrs[i] for i in perm], P_ALL)
        for k, i in enumerate(perm):
            pr = group[i]
            assert _same((q[k], lower[k], upper[k]), (pr["q"], pr["lower"], pr["upper"])) and mean[k] == pr["mean"], pr["tag"]
        q2, lower2, upper2, mean2 = sd.tail_means(distrs, P_ALL)
        assert _same(q2 + lower2 + upper2, [p[key] for key in ("q", "lower", "upper") for p in group])
        assert np.array_equal(mean2, np.array([p["mean"] for p in group]))
        for pr in group[::7]:
            alone = sd.tail_means([pr["dist"]], P_ALL)
            assert _same([alone[0][0], alone[1][0], alone[2][0]], (pr["q"], pr["lower"], pr["upper"])) and alone[3][0] == pr["mean"], pr["tag"]
    pr = [p for p in table[1] if p["case"].name == "norm12_R21" and p["kind"] == "converged" and p["quad"] == (64, 21)][0]
    d = pr["dist"]
    k = 17
    one = sd.tail_means([d], P_ALL[k:k + 1])
    assert one[0][0][0] == pr["q"][k] and one[1][0][0] == pr["lower"][k] and one[2][0][0] == pr["upper"][k]
    assert d.expected_shortfall(P_ALL[k])[0] == pr["upper"][k] and d.expected_shortfall(P_ALL[k], "lower")[0] == pr["lower"][k]
    dev = sd.tail_means([d], torch.from_numpy(P_ALL).cuda())
    for got, want in zip(dev[:3], (pr["q"], pr["lower"], pr["upper"])):
        assert isinstance(got[0], torch.Tensor) and got[0].is_cuda and got[0].shape == P_ALL.shape
        assert np.array_equal(got[0].cpu().numpy(), want, equal_nan=True)
    es = d.expected_shortfall(torch.from_numpy(P_ALL).cuda(), "lower")
    assert es.is_cuda and np.array_equal(es.cpu().numpy(), pr["lower"], equal_nan=True)
    from mlmc_amd.tool.distribution import Distribution
    old = _dist(pr["case"], pr["lam"], pr["quad"], Distribution)
    assert np.array_equal(old.expected_shortfall(P_ALL), pr["upper"], equal_nan=True)
    with pytest.raises(ValueError, match="tail must be"):
        d.expected_shortfall(0.5, "middle")


def test_groups_of_the_table_bound(hip):
    """9 Gaussian problems on a rule of 2^18 cells: four rows of 2 MiB (and 8 bytes) per problem against the table bound of 64 MiB
    put at most 8 problems into a group, so the 9 run in two groups; each is bit for bit the problem alone"""
    from mlmc_amd.tool import simple_distribution as sd
    p = np.array([0.0, 1e-3, 0.05, 0.5, 0.95, 0.999, 1.0])
    distrs = [_gaussian(0.5 * k - 2.0, 0.5 + 0.25 * k, n_intervals=1 << 18) for k in range(9)]
    assert 4 * 8 * ((1 << 18) + 1) * 9 > (64 << 20) >= 4 * 8 * ((1 << 18) + 1) * 7
    q, lower, upper, mean = sd.tail_means(distrs, p)
    for k, d in enumerate(distrs):
        alone = sd.tail_means([d], p)
        assert _same([alone[0][0], alone[1][0], alone[2][0]], (q[k], lower[k], upper[k])) and alone[3][0] == mean[k], k
        # the mean of the symmetric density: two sums of N = 2^18 x 21 positive terms, recursive-summation bound 2 (N + 8) 2^-53 (b - a)
        gate = 2 * (d.n_intervals * d._gauss_degree + 8) * U * (d.domain[1] - d.domain[0])
        assert abs(mean[k] - (0.5 * k - 2.0)) <= gate and lower[k][0] == d.domain[0] and upper[k][-1] == d.domain[1], k
    assert np.array_equal(q[8], sd.quantiles([distrs[8]], p)[0])


def test_argument_errors(hip):
    from mlmc_amd import Legendre
    lib = hip.lib()
    name = "mlmc_density_tail_means_batch"
    fn = getattr(lib, name)
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
    q, lower, upper, mass, mean = np.empty(2 * B), np.empty(2 * B), np.empty(2 * B), np.empty(B), np.empty(B)
    P = hip.ptr

    def call(**kw):
        v = dict(B=B, h=hp, r1=r1, lam=lam, sig=sig, a=a, b=b, ni=0, deg=0, p=p, n=n, q=q, lower=lower, upper=upper, mass=mass, mean=mean,
                 kind=hip.HOST)
        v.update(kw)
        return fn(v["B"], v["h"], P(v["r1"]), P(v["lam"]), P(v["sig"]), P(v["a"]), P(v["b"]), v["ni"], v["deg"], P(v["p"]), P(v["n"]),
                  P(v["q"]), P(v["lower"]), P(v["upper"]), P(v["mass"]), P(v["mean"]), v["kind"])

    def expect(rc, pattern):
        with pytest.raises(hip.MlmcHipError, match=pattern):
            hip.check(rc)
    assert call() == 0
    near = lambda x, v: np.all(np.abs(x - v) < 1e-12)                   # the uniform density on (-2, 2) at p = 0.5
    assert near(q, 0.0) and near(lower, -1.0) and near(upper, 1.0) and near(mass, 1.0) and near(mean, 0.0)
    for key in ("r1", "lam", "sig", "a", "b", "n", "p", "q", "lower", "upper"):
        expect(call(**{key: None}), name + ".*null")
    expect(call(h=None), name + ".*null")
    expect(call(B=-1), name + ".*B < 0")
    expect(call(kind=7), name + ".*mem_kind")
    expect(call(deg=65), name + ".*gauss_degree")
    expect(call(deg=-1), name + ".*gauss_degree")
    expect(call(ni=-1), name + ".*n_intervals")
    bad_b = b.copy(); bad_b[2] = dom[0]
    expect(call(b=bad_b), name + ": problem 2.*domain")
    bad_r1 = r1.copy(); bad_r1[1] = 6
    expect(call(r1=bad_r1), name + ": problem 1.*R1")
    bad_n = n.copy(); bad_n[3] = -1
    expect(call(n=bad_n), name + ": problem 3.*n < 0")
    from mlmc_amd.engine import _IdentityBasis
    id_h = (C.c_void_p * B)(*[f._basis_handle().value for f in fns])
    id_h[1] = _IdentityBasis()._basis_handle().value
    id_r1 = r1.copy(); id_r1[1] = 1
    expect(call(h=C.cast(id_h, C.c_void_p), r1=id_r1), name + ": problem 1.*unsupported basis kind")
    # no-ops: B = 0; no points at all still reports masses and means; NULL mass_out / mean_out are accepted
    assert fn(0, None, None, None, None, None, None, 0, 0, None, None, None, None, None, None, None, hip.HOST) == 0
    mass[:], mean[:] = -1.0, -7.0
    assert call(n=np.zeros(B, dtype=np.int64), p=None, q=None, lower=None, upper=None) == 0
    assert near(mass, 1.0) and near(mean, 0.0)
    assert call(mass=None, mean=None) == 0
    # a problem without points in the middle of the batch
    some = np.array([2, 0, 3, 1], dtype=np.int64)
    q[:] = 7.25
    assert call(n=some) == 0 and near(q[:6], 0.0) and np.all(q[6:] == 7.25)


# ---- Estimate ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def estimate(hip):
    """3 components, 3 levels of 2000 samples in two chunks each, Legendre(9) on the domains estimate_domains gives"""
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    from tests.test_gpu_bootstrap_batch import _memory, _root_q
    M = 3
    rng = np.random.default_rng(23)
    levels = []
    for l in range(3):
        f = (1.0 + 0.25 * np.arange(M))[:, None] * rng.normal(size=(M, 2000)) + 0.3 * np.arange(M)[:, None]
        levels.append((f, None if l == 0 else f + 0.05 * 0.5 ** l * rng.normal(size=(M, 2000))))
    st = _memory(levels, M, chunk_size=1000)
    q = _root_q(st, M)
    fns = [Legendre(9, tuple(d)) for d in Estimate.estimate_domains(q, st)]
    est = Estimate(q, st, fns[0])
    return st, q, fns, est, est.construct_densities(moments_fns=fns)


PROBS = np.array([0.01, 0.05, 0.5, 0.95, 0.99])


def test_estimate_component_shortfall(hip, estimate):
    from mlmc_amd.estimator import Estimate, scalar_component
    from mlmc_amd.tool import simple_distribution as sd
    st, q, fns, est, dens = estimate
    M = len(fns)
    wq, wl, wu, _ = sd.tail_means([d[0] for d in dens], PROBS)
    for tail, want in (("upper", wu), ("lower", wl)):
        es, qq, success = est.estimate_component_shortfall(PROBS, tail, densities=dens)
        assert es.shape == (M, PROBS.size) and qq.shape == es.shape and success.shape == (M,) and success.dtype == bool and success.all()
        assert np.array_equal(es, np.array(want)) and np.array_equal(qq, np.array(wq))
        assert np.array_equal(qq, est.estimate_component_quantiles(PROBS, densities=dens)[0])
        own, own_q, _ = est.estimate_component_shortfall(PROBS, tail, moments_fns=fns)
        assert np.array_equal(own, es) and np.array_equal(own_q, qq)
    # The scalar chain.  test_estimate_component_quantiles accepts |Fhat_m(q) - p| <= delta = 2e-5: the CDFs of the two densities
    # differ by delta.  With upper(Q(p)) = b - int_Q^b (F(t) - p) dt / (1 - p), two CDFs within delta of each other on [a, b] move
    # it by at most delta (b - a) / (1 - p) for the integrand and delta |Q_1 - Q_2| / (1 - p) <= delta (b - a) / (1 - p) for the
    # limit: 2 delta (b - a) / (1 - p); the lower tail likewise with p.
    delta, worst = 2e-5, 0.0
    for m in range(M):
        d_m = Estimate(scalar_component(q, m), st, fns[m]).construct_density(tol=1e-8, orth_moments_tol=1e-4)[0]
        width = d_m.domain[1] - d_m.domain[0]
        for tail, mass_of_tail in (("upper", 1 - PROBS), ("lower", PROBS)):
            es = est.estimate_component_shortfall(PROBS, tail, densities=dens)[0][m]
            err = np.abs(d_m.expected_shortfall(PROBS, tail) - es) / (2 * delta * width / mass_of_tail)
            worst = max(worst, float(np.max(err)))
            assert np.all(err <= 1.0), (m, tail, err)
    print(f"\ncomponent shortfall against the scalar chain: worst error / gate = {worst:.3g}")


def test_bootstrap_component_shortfall(hip, estimate):
    st, q, fns, est, dens = estimate
    M = len(fns)
    bq = est.bootstrap_component_quantiles(PROBS, 8, seed=7, moments_fns=fns, densities=dens)
    for tail in ("upper", "lower"):
        one = est.bootstrap_component_shortfall(PROBS, 8, seed=7, tail=tail, moments_fns=fns, densities=dens)
        two = est.bootstrap_component_shortfall(PROBS, 8, seed=7, tail=tail, moments_fns=fns, densities=dens)
        for x, y in zip(one, two):
            assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)
        assert one.seed == 7 and one.replicates.shape == (8, M, PROBS.size) and one.success.shape == (8, M)
        assert np.array_equal(one.q, est.estimate_component_shortfall(PROBS, tail, densities=dens)[0])
        assert np.array_equal(one.n_ok, one.success.sum(axis=0)) and one.n_ok.min() > 0
        assert np.all(one.lo <= one.hi)
        # the same replicate densities as the quantile bands: the same verdicts, and the shortfall beyond each quantile
        assert np.array_equal(one.success, bq.success)
        both = one.success & bq.success
        if tail == "upper":
            assert np.all(one.replicates[both] >= bq.replicates[both])
        else:
            assert np.all(one.replicates[both] <= bq.replicates[both])
    again = est.bootstrap_component_quantiles(PROBS, 8, seed=7, moments_fns=fns, densities=dens)
    assert np.array_equal(again.replicates, bq.replicates) and np.array_equal(again.q, bq.q)
