"""GPU tests of the batched expectations under the max-entropy densities (k_q_moments in mlmc_amd/csrc/density.hip) through the
public entries: simple_distribution.density_moments / summaries, the fitted_moments / summary / entropy methods,
Estimate.estimate_component_summaries / bootstrap_component_summaries and mlmc_density_moments_batch.

Moments, mass and entropy (include/mlmc_hip.h) are finite sums; tests/density_moment_cases.py evaluates them in 80-bit long double.
The main test requires |value - reference| <= tol_units 2^-53 scale, tol_units = 4 x the worst error of the fp64 twin on the CPU
(mm.TWIN_UNITS_M, tests/test_density_moments_cpu.py), at least 16.  The worst units per tolerance class and column are printed
before the assertion (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

from tests import density_moment_cases as mm
from tests import maxent_cases as mc
from tests import maxent_exact as mx
from tests import quantile_cases as qc
from tests.test_gpu_divergences import EXP_DOMAIN, EXP_PAIRS, _exp_integral, _exponential
from tests.test_gpu_quantiles import _dist, _fn
from tests.test_gpu_tail_means import estimate      # noqa: F401 (the fixture of the Estimate-level tests)

pytestmark = pytest.mark.gpu
LD = np.longdouble
U = 2.0 ** -53
NAME = "mlmc_density_moments_batch"


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


_TEST_FNS = {}


def _test_fn(desc):
    """the package's moments object of a test-basis description"""
    key = (desc.kind, desc.size, desc.domain, desc.ref_domain, desc.log, None if desc.matrix is None else desc.matrix.tobytes())
    if key not in _TEST_FNS:
        import mlmc_amd
        cls = {mx.LEGENDRE: mlmc_amd.Legendre, mx.MONOMIAL: mlmc_amd.Monomial, mx.FOURIER: mlmc_amd.Fourier, mx.SPLINE: mlmc_amd.Spline}[desc.kind]
        base = cls(desc.size, desc.domain, ref_domain=desc.ref_domain, log=desc.log)
        assert float(base._linear_scale) == desc.scale and float(base._linear_shift) == desc.shift
        _TEST_FNS[key] = base if desc.matrix is None else mlmc_amd.TransformedMoments(base, desc.matrix)
    return _TEST_FNS[key]


def _raw(distrs, fns, ks, quad=None):
    """mlmc_density_moments_batch itself: (out [B, Kmax], mass [B], entropy [B]), pre-filled with -7"""
    from mlmc_amd import _lib
    from mlmc_amd.tool import simple_distribution as sd
    B = len(distrs)
    handles, r1, lam, sig = sd._batch_problem_args(distrs)
    a = np.array([float(d.domain[0]) for d in distrs])
    b = np.array([float(d.domain[1]) for d in distrs])
    tests = (C.c_void_p * B)(*[fn._basis_handle().value for fn in fns])
    ks = np.ascontiguousarray(ks, dtype=np.int32)
    quad = (distrs[0].n_intervals, distrs[0]._gauss_degree) if quad is None else quad
    out, mass, ent = np.full((B, int(ks.max())), -7.0), np.full(B, -7.0), np.full(B, -7.0)
    _lib.check(_lib.lib().mlmc_density_moments_batch(B, C.cast(handles, C.c_void_p), _lib.ptr(r1), _lib.ptr(lam), _lib.ptr(sig),
                                                     _lib.ptr(a), _lib.ptr(b), quad[0], quad[1], C.cast(tests, C.c_void_p), _lib.ptr(ks),
                                                     _lib.ptr(out), _lib.ptr(mass), _lib.ptr(ent)))
    return out, mass, ent


def _cdf_mass(distrs):
    from mlmc_amd.tool import simple_distribution as sd
    return sd._on_rule(distrs, [np.array([0.5])] * len(distrs), False, "cdfs_on_rule")[1]


@pytest.fixture(scope="module")
def converged(hip):
    """name -> the multipliers the device solver returns on the default rule at tol = 1e-8"""
    from mlmc_amd.tool import simple_distribution as sd
    out = {}
    for case in mc.cases().values():
        lam, _, _, info = sd._solve_on_device(_fn(case), case.mu, case.sigma, case.domain, case.lam0, 1e-8, 100, n_intervals=64,
                                              gauss_degree=21)
        assert info.success == 1, case.name
        out[case.name] = lam
    return out


@pytest.fixture(scope="module")
def table(hip, converged):
    """per rule: the problems (case, multipliers, test basis) of mm.rules_and_bases and ONE call of the entry over all of them,
    shared by the tests"""
    rules = {}
    for case in mc.cases().values():
        for kind, lam in (("converged", converged[case.name]), ("perturbed", mc.perturbed(converged[case.name]))):
            for quad, name in mm.rules_and_bases(case):
                desc, K = mm.bases_of(case)[name]
                rules.setdefault(quad, []).append(dict(case=case, kind=kind, lam=lam, base=name, desc=desc, K=K, quad=quad,
                                                       tag=f"{case.name} {kind} {name} {quad[0]}x{quad[1]}"))
    out = []
    for quad, probs in rules.items():
        distrs = [_dist(p["case"], p["lam"], quad) for p in probs]
        fns = [_test_fn(p["desc"]) for p in probs]
        ks = np.array([p["K"] for p in probs], dtype=np.int32)
        got = _raw(distrs, fns, ks)
        out.append(dict(quad=quad, probs=probs, distrs=distrs, fns=fns, ks=ks, got=got))
    return out


def test_accuracy(table):
    """moments, mass and entropy of every problem of the table against the long-double reference"""
    failures, worst, n = [], {}, 0
    for t in table:
        out, mass, ent = t["got"]
        for i, p in enumerate(t["probs"]):
            ref, scale = mm.moment_sums(p["case"], p["lam"], p["desc"], p["K"], p["quad"])
            assert np.all(out[i, p["K"]:] == 0.0), p["tag"]
            got = dict(moments=out[i, :p["K"]], mass=mass[i], entropy=ent[i])
            cls = mc.tolerance_class(p["case"])
            for col, v in mm.worst_units(got, ref, scale).items():
                n += 1
                tol = mm.moment_tolerance(cls, col, p["kind"])
                if v > worst.get((cls, p["kind"], col), (-1.0, None))[0]:
                    worst[(cls, p["kind"], col)] = (v, p["tag"])
                if not v <= tol:
                    failures.append(f"{p['tag']}: {col} is {v:.4g} units off (tolerance {tol:g})")
    print()
    for (cls, kind, col), (v, where) in sorted(worst.items()):
        print(f"worst {cls:8s} {kind:9s} {col:8s} {v:10.4g} units at {where} (twin {mm.TWIN_UNITS_M[(cls, kind)][col]:g})")
    assert n > 3000
    assert not failures, "\n".join(failures[:40])


def test_mass_is_the_mass_of_the_cdf_entry(table):
    """mass_out is bit for bit the mass of mlmc_density_cdf_batch for every problem and rule"""
    for t in table:
        assert np.array_equal(t["got"][1], _cdf_mass(t["distrs"])), t["quad"]


def test_batch_independence(table):
    """a problem alone, first, last, among problems of other K and other families, and permuted: the same bits (the entry has no
    groups: one launch serves every problem of a call)"""
    rng = np.random.default_rng(5)
    for t in table:
        distrs, fns, ks, (out, mass, ent) = t["distrs"], t["fns"], t["ks"], t["got"]
        B = len(distrs)
        perm = rng.permutation(B)
        o2, m2, e2 = _raw([distrs[i] for i in perm], [fns[i] for i in perm], ks[perm])
        assert np.array_equal(o2, out[perm], equal_nan=True) and np.array_equal(m2, mass[perm]) and np.array_equal(e2, ent[perm])
        for i in list(range(0, B, 37)) + [B - 1]:
            o1, m1, e1 = _raw([distrs[i]], [fns[i]], ks[i:i + 1])
            assert np.array_equal(o1[0], out[i, :ks[i]], equal_nan=True) and m1[0] == mass[i] and e1[0] == ent[i], t["probs"][i]["tag"]
            j = (i + 11) % B                             # first and last of a pair with another problem (another Kmax, another LDS layout)
            for order in ((i, j), (j, i)):
                o3, m3, e3 = _raw([distrs[k] for k in order], [fns[k] for k in order], ks[list(order)])
                at = order.index(i)
                assert np.array_equal(o3[at, :ks[i]], out[i, :ks[i]], equal_nan=True) and m3[at] == mass[i] and e3[at] == ent[i]
    # fewer outputs than the basis has: K of a plain basis truncates the generator, K of a matrix basis selects rows
    t = table[0]
    for i in (k for k, p in enumerate(t["probs"]) if p["kind"] == "converged" and p["case"].name in ("norm12_R21", "mix_R9")):
        out = t["got"][0]
        for K in (1, 2, int(t["ks"][i]) - 1):
            o1, m1, e1 = _raw([t["distrs"][i]], [t["fns"][i]], [K])
            assert o1.shape == (1, K) and np.array_equal(o1[0], out[i, :K]) and m1[0] == t["got"][1][i] and e1[0] == t["got"][2][i]


def test_fitted_moments(hip):
    """solved distributions with unit mean of the constant: the normalised fitted moments meet
    |m_i - mu_i| / sigma_i <= 2 tol (2 + max |mu / sigma|), from grad_norm < tol and |moment0 - 1| <= tol of the normalisation fix"""
    from mlmc_amd.tool import simple_distribution as sd
    tol = 1e-8
    cases = [c for c in mc.cases().values() if abs(c.mu[0] - 1.0) <= 1e-12 and c.sigma[0] <= 1.0]
    assert len(cases) >= 6
    distrs = [sd.SimpleDistribution(_fn(c), np.stack([c.mu, c.sigma ** 2], axis=1), domain=c.domain) for c in cases]
    results = sd.estimate_densities_minimize(distrs, tol)
    res = sd.density_moments(distrs)
    n = 0
    for c, d, r, m in zip(cases, distrs, results, res.moments):
        if not r.success:
            continue
        n += 1
        err = np.abs(m - c.mu) / c.sigma
        bound = 2 * tol * (2 + np.max(np.abs(c.mu / c.sigma)))
        print(f"\n{c.name}: worst fitted-moment error {np.max(err):.3g} (bound {bound:.3g})")
        assert m.shape == (c.R1,) and np.all(err <= bound), (c.name, err, bound)
        assert np.array_equal(d.fitted_moments(), m)
    assert n >= 6


def _uniform(dom, quad=(64, 21)):
    import mlmc_amd
    from mlmc_amd.tool import simple_distribution as sd
    d = sd.SimpleDistribution(mlmc_amd.Legendre(2, dom), np.stack([np.eye(2)[0], np.ones(2)], axis=1), domain=dom)
    d.multipliers, d._moment_errs = np.array([np.log(dom[1] - dom[0]), 0.0]), np.ones(2)
    d.n_intervals, d._gauss_degree = quad
    return d


# the statistics are smooth functions of five normalised moments, each within tol_units 2^-53 of its scale (<= 1 here); the
# divisions by c2^(3/2) and c2^2 amplify by at most 12^2 = 144 for the densities below (c2 >= 1/12 in units of W^2) and the
# formulas have at most 8 terms: 16 x 2^-53 x 144 x 8 = 2e-12
STAT_RTOL = 4e-12


def test_uniform_closed_form(hip):
    import mlmc_amd
    from mlmc_amd.tool import simple_distribution as sd
    tol = mm.moment_tolerance("regular", "moments")
    for dom in ((-4.0, 6.0), (0.5, 3.0), (-7.0, -2.0)):
        d = _uniform(dom)
        W = dom[1] - dom[0]
        case = mc.Case("uniform", mx.Desc(mx.LEGENDRE, 2, dom), np.eye(2)[0], np.ones(2), d.multipliers, "other")
        desc = mx.Desc(mx.LEGENDRE, 8, dom)
        out, mass, ent = _raw([d], [_test_fn(desc)], [8])
        _, scale = mm.moment_sums(case, d.multipliers, desc, 8, (64, 21))
        want = dict(moments=np.eye(8)[0].astype(LD), mass=LD(1), entropy=np.log(LD(W)))
        u = mm.worst_units(dict(moments=out[0], mass=mass[0], entropy=ent[0]), want, scale)
        print(f"\nuniform {dom}: units {u}")
        assert all(v <= tol for v in u.values()), (dom, u)
        s = d.summary()
        assert abs(s.mean - 0.5 * (dom[0] + dom[1])) <= STAT_RTOL * max(abs(dom[0]), abs(dom[1]))
        assert abs(s.var - W * W / 12) <= STAT_RTOL * W * W and abs(s.skewness) <= STAT_RTOL and abs(s.kurtosis - 1.8) <= STAT_RTOL
        assert abs(s.entropy - np.log(W)) <= STAT_RTOL * max(1.0, abs(np.log(W))) and abs(s.mass - 1) <= STAT_RTOL
        assert s.entropy == d.entropy()


def test_exponential_closed_form(hip):
    """R1 = 2: rho = exp(-(c0 + c1 x)) has elementary integrals for the mass, the entropy column int rho (c0 + c1 x) and the
    monomial moments; the truncation error of the 21-point rule on cells of width 1/8 at these slopes is far below one unit"""
    lo, hi = EXP_DOMAIN
    tol = mm.moment_tolerance("regular", "moments")
    desc = mx.Desc(mx.MONOMIAL, 2, EXP_DOMAIN)                       # t = (x + 4) / 8
    for kind, lam_p, lam_q in EXP_PAIRS:
        for lam in (lam_p, lam_q):
            case, c0, c1 = _exponential(kind, lam)
            i0, i1 = _exp_integral(c0, c1, lo, hi), _exp_integral(c0, c1, lo, hi, 1)
            want = dict(moments=np.array([i0, (i1 + 4 * i0) / 8], dtype=LD), mass=i0, entropy=c0 * i0 + c1 * i1)
            d = _dist(case, case.lam0, (64, 21))
            out, mass, ent = _raw([d], [_test_fn(desc)], [2])
            _, scale = mm.moment_sums(case, case.lam0, desc, 2, (64, 21))
            u = mm.worst_units(dict(moments=out[0], mass=mass[0], entropy=ent[0]), want, scale)
            print(f"\nexponential {kind} {lam}: units {u}")
            assert all(v <= tol for v in u.values()), (kind, lam, u)
            s = d.summary()
            assert abs(s.mean - float(i1 / i0)) <= STAT_RTOL * 4.0 and s.mass == mass[0]
            assert abs(s.entropy - float((c0 * i0 + c1 * i1) / i0 + np.log(i0))) <= STAT_RTOL * 8.0


# ---- specials ---------------------------------------------------------------------------------------------------------------------
def test_nan_rows(table, converged):
    """NaN multipliers: every output of the problem NaN; a test basis with a narrower clipped domain: moments NaN, mass and entropy
    as before; the other problems of the call as before; no error"""
    import mlmc_amd
    from mlmc_amd.tool import simple_distribution as sd
    case = mc.cases()["mix_R9"]
    lam = converged["mix_R9"]
    good = _dist(case, lam, (64, 21))
    bad = lam.copy()
    bad[2] = np.nan
    nan_lam = _dist(case, bad, (64, 21))
    wide = _dist(case, lam, (64, 21))
    wide.domain = (case.domain[0] - 1.0, case.domain[1])            # nodes outside the domain of the density's basis
    leg = mlmc_amd.Legendre(8, case.domain)
    narrow = mlmc_amd.Legendre(8, (case.domain[0] + 1.0, case.domain[1]))
    open_ = mlmc_amd.Legendre(8, (case.domain[0] + 1.0, case.domain[1]), safe_eval=False)
    out, mass, ent = _raw([good, nan_lam, good, wide, good, good], [leg, leg, narrow, leg, open_, leg], [8, 8, 8, 8, 8, 3])
    o1, m1, e1 = _raw([good], [leg], [8])
    assert np.all(np.isfinite(o1)) and m1[0] > 0
    assert np.array_equal(out[0], o1[0]) and np.array_equal(out[5, :3], o1[0, :3]) and np.all(out[5, 3:] == 0)
    assert np.all(np.isnan(out[1])) and np.isnan(mass[1]) and np.isnan(ent[1])
    assert np.all(np.isnan(out[3])) and np.isnan(mass[3]) and np.isnan(ent[3])
    assert np.all(np.isnan(out[2])) and np.all(np.isfinite(out[4]))
    assert np.all(mass[[0, 2, 4, 5]] == m1[0]) and np.all(ent[[0, 2, 4, 5]] == e1[0])
    res = sd.density_moments([good, nan_lam], narrow)
    assert all(np.all(np.isnan(m)) for m in res.moments) and np.isfinite(res.entropy[0]) and np.isnan(res.entropy[1])
    s = sd.summaries([good, nan_lam])
    assert all(np.isfinite(v[0]) and np.isnan(v[1]) for v in s)


def test_clipped_exponents(converged):
    """mc.clip_multipliers: the entropy uses the clipped exponent; all columns within the tolerance of the regular class at
    multipliers away from a normalised density"""
    quad = (64, 21)
    for name in mc.CLIP_CASES:
        case = mc.cases()[name]
        lc = mc.clip_multipliers(case, converged[name])
        for base in ("own", "legendre8", "fourier9"):
            desc, K = mm.bases_of(case)[base]
            exps = []
            ref, scale = mm.moment_sums(case, lc, desc, K, quad, exponents=exps)
            mc.assert_clip_band(exps[0])
            assert np.max(exps[0]) > 200 and np.min(exps[0]) < -200
            out, mass, ent = _raw([_dist(case, lc, quad)], [_test_fn(desc)], [K])
            u = mm.worst_units(dict(moments=out[0], mass=mass[0], entropy=ent[0]), ref, scale)
            print(f"\nclipped {name} {base}: units {u}")
            assert all(v <= mm.moment_tolerance("regular", col, "perturbed") for col, v in u.items()), (name, base, u)


def test_argument_errors(hip):
    from mlmc_amd import Legendre, Monomial
    from mlmc_amd.tool import simple_distribution as sd
    lib = hip.lib()
    fn = getattr(lib, NAME)
    B = 4
    doms = [(-2.0, 2.0), (-2.0, 2.0), (-1.0, 3.0), (2.0, 5.0)]
    fns = [Legendre(5, dom) for dom in doms]
    tfn = [Monomial(4, dom) for dom in doms]
    handles = (C.c_void_p * B)(*[f._basis_handle().value for f in fns])
    tests = (C.c_void_p * B)(*[f._basis_handle().value for f in tfn])
    r1 = np.full(B, 5, dtype=np.int32)
    ks = np.array([4, 1, 3, 2], dtype=np.int32)
    lam, sig = np.zeros((B, 5)), np.ones((B, 5))
    lam[:, 0] = np.log(4.0)
    a, b = np.array([d[0] for d in doms]), np.array([d[1] for d in doms])
    out, mass, ent = np.empty((B, 4)), np.empty(B), np.empty(B)
    Pt = hip.ptr

    def call(**kw):
        v = dict(B=B, h=C.cast(handles, C.c_void_p), r1=r1, lam=lam, sig=sig, a=a, b=b, ni=0, deg=0, t=C.cast(tests, C.c_void_p), k=ks,
                 out=out, mass=mass, ent=ent)
        v.update(kw)
        ptr = lambda x: x if x is None or isinstance(x, C.c_void_p) else Pt(x)
        return fn(v["B"], v["h"], ptr(v["r1"]), ptr(v["lam"]), ptr(v["sig"]), ptr(v["a"]), ptr(v["b"]), v["ni"], v["deg"], v["t"],
                  ptr(v["k"]), ptr(v["out"]), ptr(v["mass"]), ptr(v["ent"]))

    def expect(rc, pattern):
        with pytest.raises(hip.MlmcHipError, match=pattern):
            hip.check(rc)
    assert call() == 0
    # uniform densities 1/4 on domains of width 4, 4, 4 and 3: monomial moments W / (4 (k + 1)) of t in (0, 1), zeros beyond K
    W = b - a
    for i in range(B):
        assert np.all(np.abs(out[i, :ks[i]] - W[i] / 4 / (1 + np.arange(ks[i]))) < 1e-14) and np.all(out[i, ks[i]:] == 0)
    assert np.all(np.abs(mass - W / 4) < 1e-14) and np.all(np.abs(ent - W / 4 * np.log(4.0)) < 1e-14)
    assert call(mass=None, ent=None) == 0
    for key in ("r1", "lam", "sig", "a", "b", "k", "out", "h", "t"):
        expect(call(**{key: None}), NAME + ".*null")
    expect(call(B=-1), NAME + ".*B < 0")
    expect(call(deg=65), NAME + ".*gauss_degree")
    expect(call(deg=-1), NAME + ".*gauss_degree")
    expect(call(ni=-1), NAME + ".*n_intervals")
    expect(call(ni=(1 << 20) + 1), NAME + ".*n_intervals")
    bad_b = b.copy(); bad_b[2] = a[2]
    expect(call(b=bad_b), NAME + ": problem 2.*domain")
    nan_a = a.copy(); nan_a[0] = np.nan
    expect(call(a=nan_a), NAME + ": problem 0.*domain")
    bad_r1 = r1.copy(); bad_r1[1] = 6
    expect(call(r1=bad_r1), NAME + ": problem 1.*R1")
    for i, k in ((0, 5), (3, 0), (1, -1)):
        bad_k = ks.copy(); bad_k[i] = k
        expect(call(k=bad_k), NAME + f": problem {i}: K out of range")
    from mlmc_amd.engine import _IdentityBasis
    ident = _IdentityBasis()
    bad_t = (C.c_void_p * B)(*[f._basis_handle().value for f in tfn])
    bad_t[2] = None
    expect(call(t=C.cast(bad_t, C.c_void_p)), NAME + ": problem 2: null test basis")
    bad_t[2] = ident._basis_handle().value
    one_k = ks.copy(); one_k[2] = 1
    expect(call(t=C.cast(bad_t, C.c_void_p), k=one_k), NAME + ": problem 2: unsupported test basis kind")
    bad_h = (C.c_void_p * B)(*[f._basis_handle().value for f in fns])
    bad_h[1] = ident._basis_handle().value
    one_r = r1.copy(); one_r[1] = 1
    expect(call(h=C.cast(bad_h, C.c_void_p), r1=one_r), NAME + ": problem 1.*unsupported basis kind")
    # no-ops
    out[:] = 7.25
    assert fn(0, None, None, None, None, None, None, 0, 0, None, None, None, None, None) == 0 and np.all(out == 7.25)
    empty = sd.density_moments([])
    assert empty.moments == [] and empty.entropy.shape == (0,) and empty.mass.shape == (0,)
    assert all(v.shape == (0,) for v in sd.summaries([]))


# ---- the Python entries -----------------------------------------------------------------------------------------------------------
def test_python_entries(table):
    """density_moments is the entry with the normalisation on top; summaries is bit for bit the objects' summary()"""
    from mlmc_amd.tool import simple_distribution as sd
    from mlmc_amd.tool.distribution import Distribution
    t = table[0]
    sel = [i for i, p in enumerate(t["probs"]) if p["base"] in ("own", "fourier9") and p["kind"] == "converged"]
    distrs, fns, ks = [t["distrs"][i] for i in sel], [t["fns"][i] for i in sel], t["ks"][sel]
    out, mass, ent = (v[sel] for v in t["got"])
    raw = sd.density_moments(distrs, fns, [int(k) for k in ks], normalize=False)
    res = sd.density_moments(distrs, fns, [int(k) for k in ks])
    assert np.array_equal(raw.mass, mass) and np.array_equal(res.mass, mass) and np.array_equal(raw.entropy, ent)
    assert np.array_equal(res.entropy, ent / mass + np.log(mass))
    for i in range(len(sel)):
        assert np.array_equal(raw.moments[i], out[i, :ks[i]]) and np.array_equal(res.moments[i], out[i, :ks[i]] / mass[i])
    own = [i for i, k in enumerate(sel) if t["probs"][k]["base"] == "own"]
    fitted = sd.density_moments([distrs[i] for i in own])
    for i, m in zip(own, fitted.moments):
        assert np.array_equal(m, res.moments[i]) and np.array_equal(distrs[i].fitted_moments(), m)
    one = sd.density_moments([distrs[i] for i in own], fns[own[0]], 2)       # one object, one size for all
    assert all(m.shape == (2,) for m in one.moments)
    every = sd.summaries(distrs)
    assert np.array_equal(every.mass, mass) and np.array_equal(every.entropy, res.entropy)
    for i in range(0, len(distrs), 7):
        s = distrs[i].summary()
        assert isinstance(s, sd.DensitySummary) and all(isinstance(v, float) for v in s)
        assert np.array_equal(np.array(s), np.array([v[i] for v in every]))
        assert distrs[i].entropy() == s.entropy
    p = t["probs"][sel[0]]
    old = _dist(p["case"], p["lam"], p["quad"], Distribution)
    assert np.array_equal(np.array(old.summary()), np.array([v[0] for v in every])) and np.array_equal(old.fitted_moments(), res.moments[0])
    assert old.entropy() == every.entropy[0]
    # the converged densities have the statistics of their targets: the two-Gaussian mixture of the mix cases
    k = [i for i, j in enumerate(sel) if t["probs"][j]["case"].name == "mix_R26" and t["probs"][j]["base"] == "own"][0]
    mean = 0.6 * 0.5 + 0.4 * 2.5
    var = 0.6 * (1.0 + 0.5 ** 2) + 0.4 * (0.49 + 2.5 ** 2) - mean ** 2
    assert abs(every.mean[k] - mean) < 1e-3 and abs(every.var[k] - var) < 1e-2


def test_estimate_component_summaries(hip, estimate):
    from mlmc_amd.tool import simple_distribution as sd
    st, q, fns, est, dens = estimate
    res = est.estimate_component_summaries(densities=dens)
    assert isinstance(res, sd.DensitySummary) and all(v.shape == (len(fns),) for v in res)
    for m, d in enumerate(dens):
        assert np.array_equal(np.array(d[0].summary()), np.array([v[m] for v in res]))
    # component m is 0.3 m + (1 + 0.25 m) N(0, 1) on a domain cut at its 1 % and 99 % quantiles: between the uniform and the
    # Gaussian kurtosis, or a little above
    assert np.all(np.abs(res.mass - 1) < 1e-6) and np.all(np.abs(res.skewness) < 0.5) and np.all((res.kurtosis > 1.8) & (res.kurtosis < 4.0))
    assert np.all(np.abs(res.mean - 0.3 * np.arange(3)) < 0.2) and np.all(res.var > 0.5)
    again = est.estimate_component_summaries(moments_fns=fns)
    for x, y in zip(res, again):
        assert np.array_equal(x, y)


def test_bootstrap_component_summaries(hip, estimate):
    from mlmc_amd.estimator import QuantileBands, quantile_bands
    from mlmc_amd.tool import simple_distribution as sd
    st, q, fns, est, dens = estimate
    M, B, R = len(fns), 8, 9
    one = est.bootstrap_component_summaries(B, seed=7, level=0.8, moments_fns=fns, densities=dens)
    two = est.bootstrap_component_summaries(B, seed=7, level=0.8, densities=dens)
    assert isinstance(one, QuantileBands) and one.seed == 7
    for x, y in zip(one, two):
        assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)
    assert one.q.shape == (M, 5) and one.replicates.shape == (B, M, 5) and one.lo.shape == one.hi.shape == (M, 5)
    assert np.array_equal(one.q, np.stack(est.estimate_component_summaries(densities=dens)[:5], axis=1))
    lo, hi = quantile_bands(one.replicates, one.success, 0.8)
    assert np.array_equal(one.lo, lo) and np.array_equal(one.hi, hi) and np.all(one.lo <= one.hi)
    bq = est.bootstrap_component_quantiles(np.array([0.05, 0.5, 0.95]), B, seed=7, moments_fns=fns, densities=dens)
    assert np.array_equal(one.success, bq.success) and np.array_equal(one.n_ok, bq.n_ok) and one.n_ok.min() > 0
    # the same chain from public pieces
    reps = est.est_bootstrap_components(B, moments_fns=fns, seed=7)
    distrs = []
    for b in range(B):
        for m in range(M):
            mobj = dens[m][3]
            mu = np.sum([reps.l_means[b, l, m, :R] @ mobj._base_matrix.T for l in range(reps.l_means.shape[1])], axis=0)
            distrs.append(sd.SimpleDistribution(mobj, np.stack((mu, np.ones(mobj.size)), axis=1), domain=mobj.domain))
    sd.estimate_densities_minimize(distrs, 1e-8, 0.0)
    want = np.stack(sd.summaries(distrs)[:5], axis=1).reshape(B, M, 5)
    assert np.array_equal(one.replicates, want, equal_nan=True)
    # a replicate of a few thousand samples stays close to the estimate
    ok = one.success
    assert np.all(np.abs(one.replicates[..., 0] - one.q[None, :, 0])[ok] < 0.3)
