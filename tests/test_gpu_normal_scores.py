"""GPU tests of the normal scores of stored samples (k_q_scores in mlmc_amd/csrc/density.hip) through mlmc_density_scores_batch,
simple_distribution.normal_scores, quantity_estimate.component_covariance(scores=...), Estimate.estimate_score_correlation and
Estimate.sample_joint(corr="scores").

z = normcdfinv(clamp(Fhat(x))), NaN for NaN and outside the open domain (include/mlmc_hip.h).  u is compared bit for bit with
mlmc_density_cdf_batch, z with mpmath at the device's own u, both with the closed forms of tests/score_cases.py; the accumulation
with long-double sums of the device's own scores."""
import ctypes as C
import os
import types

import numpy as np
import pytest
from scipy import special

from tests import joint_sample_cases as jc
from tests import maxent_cases as mc
from tests import quantile_cases as qc
from tests import score_cases as sk
from tests.test_gpu_density_samples import CASES
from tests.test_gpu_quantiles import _dist, _fn, _raw_args

pytestmark = pytest.mark.gpu
NAME = "mlmc_density_scores_batch"
LD = np.longdouble
U = sk.U
M_SET = (1, 2, 3, 17, 65)
N_SET = (0, 1, 15, 63, 64, 65, 255, 257, 1000)
PAD = 7.25


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


@pytest.fixture(scope="module")
def table(hip):
    """per rule of qc.RULES the six cases of the sampling tests at the multipliers the device solver returns at tol = 1e-8"""
    from mlmc_amd.tool import simple_distribution as sd
    out = []
    for quad in qc.RULES:
        group = []
        for name in CASES:
            case = mc.cases()[name]
            lam, _, _, info = sd._solve_on_device(_fn(case), case.mu, case.sigma, case.domain, case.lam0, 1e-8, 100,
                                                  n_intervals=quad[0], gauss_degree=quad[1])
            assert info.success == 1, (name, quad)
            group.append(dict(case=case, lam=lam, quad=quad, dist=_dist(case, lam, quad), tag=f"{name} {quad[0]}x{quad[1]}"))
        out.append(group)
    return out


def _cycle(group, M):
    return [group[i % len(group)] for i in range(M)]


def _closed(rate, dom, quad=(64, 21)):
    """the truncated exponential of tests/score_cases.py as a distribution object"""
    return sk.closed_distribution(rate, dom, quad)


def _closed_three(quad=(64, 21)):
    return [_closed(r, d, quad) for r, d in zip(sk.RATES, sk.DOMAINS)]


def _points(rng, group, n, outside=True):
    """[M, n] values: mostly inside each problem's domain, some near the ends, and (outside) a few NaN and out-of-domain ones"""
    x = np.empty((len(group), n))
    for m, p in enumerate(group):
        a, b = p["dist"].domain if "dist" in p else p["domain"]
        row = a + (b - a) * rng.random(n)
        if n > 4:
            row[1] = a + (b - a) * 1e-9
            row[2] = b - (b - a) * 1e-9
        if outside and n > 8:
            row[(3 + m) % n] = np.nan
            row[(5 + 2 * m) % n] = b + 0.25 * (b - a)
            row[(7 + 3 * m) % n] = a - 1e-3 * (b - a)
        x[m] = row
    return x


def _problem_args(hip, group, domains=None):
    handles, r1, lam, sig = _raw_args(hip, group)
    doms = [p["dist"].domain for p in group] if domains is None else domains
    a = np.array([float(d[0]) for d in doms], dtype=np.float64)
    b = np.array([float(d[1]) for d in doms], dtype=np.float64)
    return handles, r1, lam, sig, a, b


def _scores(hip, group, fine, coarse=None, ld_in=None, ld_out=None, want_u=True, want_mass=False, quad=None, domains=None):
    """mlmc_density_scores_batch on device copies of fine / coarse [M, n] with rows ld_in apart; the outputs have rows ld_out apart
    and are returned as NumPy [M, n] after the columns beyond n have been checked to be untouched: (rc, zf, zc, uf, uc, mass)"""
    import torch
    M, n = fine.shape
    ld_in = n if ld_in is None else ld_in
    ld_out = n if ld_out is None else ld_out

    def up(x):
        if x is None:
            return None
        t = torch.full((M, ld_in), np.nan, dtype=torch.float64, device="cuda")
        t[:, :n] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        return t

    def out(want):
        return torch.full((M, ld_out), PAD, dtype=torch.float64, device="cuda") if want else None
    f, c = up(fine), up(coarse)
    zf, zc, uf, uc = out(True), out(coarse is not None), out(want_u), out(want_u and coarse is not None)
    torch.cuda.synchronize()
    handles, r1, lam, sig, a, b = _problem_args(hip, group, domains)
    mass = np.full(M, -1.0) if want_mass else None
    quad = group[0]["quad"] if quad is None else quad
    rc = hip.lib().mlmc_density_scores_batch(M, C.cast(handles, C.c_void_p), hip.ptr(r1), hip.ptr(lam), hip.ptr(sig), hip.ptr(a), hip.ptr(b),
                                             quad[0], quad[1], hip.ptr(f), hip.ptr(c), n, ld_in, hip.ptr(zf), hip.ptr(zc), ld_out,
                                             hip.ptr(uf), hip.ptr(uc), hip.ptr(mass))

    def down(t):
        if t is None:
            return None
        h = t.cpu().numpy()
        assert np.all(h[:, n:] == PAD), "columns beyond n were written"
        return np.ascontiguousarray(h[:, :n])
    return rc, down(zf), down(zc), down(uf), down(uc), mass


def _ok(hip, *args, **kw):
    res = _scores(hip, *args, **kw)
    hip.check(res[0])
    return res[1:] if kw.get("want_mass") else res[1:5]


def _cdf(hip, group, x, quad=None, domains=None):
    """mlmc_density_cdf_batch at x [M, n] (host arrays): (Fhat [M, n], mass [M])"""
    M, n = x.shape
    handles, r1, lam, sig, a, b = _problem_args(hip, group, domains)
    pts = np.ascontiguousarray(x, dtype=np.float64)
    counts = np.full(M, n, dtype=np.int64)
    out, mass = np.full(pts.shape, PAD), np.full(M, -1.0)
    quad = group[0]["quad"] if quad is None else quad
    hip.check(hip.lib().mlmc_density_cdf_batch(M, C.cast(handles, C.c_void_p), hip.ptr(r1), hip.ptr(lam), hip.ptr(sig), hip.ptr(a), hip.ptr(b),
                                               quad[0], quad[1], hip.ptr(pts), hip.ptr(counts), hip.ptr(out), hip.ptr(mass), hip.HOST))
    return out, mass


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _kept(group, x, domains=None):
    doms = [p["dist"].domain for p in group] if domains is None else domains
    return np.array([(row > d[0]) & (row < d[1]) for row, d in zip(x, doms)]).reshape(x.shape)


def _check_against_cdf(hip, group, x, z, u, quad=None, domains=None):
    """u is bit for bit the CDF entry's value at every kept point and NaN elsewhere; z is NaN exactly where u is and otherwise the
    device's normcdfinv of the clamped u: monotone in u, within the clamp's range"""
    keep = _kept(group, x, domains)
    want, _ = _cdf(hip, group, x, quad, domains)
    assert np.all(np.isnan(u[~keep])) and np.all(np.isnan(z[~keep]))
    assert _bits(u[keep], want[keep])
    assert np.array_equal(np.isnan(z), np.isnan(u))
    fin = np.isfinite(u)
    assert np.all(np.abs(z[fin]) <= 8.3)
    ref = special.ndtri(np.minimum(np.maximum(u[fin], sk.U_LO), sk.U_HI))
    # SciPy's ndtri within its 16 units of mpmath (tests/test_joint_samples_cpu.py) plus the device's tolerance; the check against
    # mpmath itself is test_scores_against_mpmath
    assert np.all(np.abs(z[fin] - ref) <= (16 + sk.z_tolerance()) * U * np.maximum(1.0, np.abs(ref)))


@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("M", M_SET)
def test_uniforms_bit_for_bit(hip, table, rule, M):
    """every n of N_SET, ld_in / ld_out in {n, n + 3}, with and without coarse: u_fine / u_coarse == mlmc_density_cdf_batch at the
    same values for every kept point, NaN elsewhere; nothing beyond column n is written; the masses are the CDF entry's"""
    rng = np.random.default_rng(1000 * rule + M)
    group = _cycle(table[rule], M)
    for n in N_SET:
        fine = _points(rng, group, n)
        coarse = _points(rng, group, n)
        for pad_in, pad_out, with_coarse in ((0, 0, True), (3, 0, False), (0, 3, False), (3, 3, True)):
            zf, zc, uf, uc, mass = _ok(hip, group, fine, coarse if with_coarse else None, ld_in=n + pad_in, ld_out=n + pad_out, want_mass=True)
            assert zf.shape == (M, n)
            assert np.array_equal(mass, _cdf(hip, group, np.zeros((M, 0)))[1])
            if n == 0:
                continue
            _check_against_cdf(hip, group, fine, zf, uf)
            if with_coarse:
                _check_against_cdf(hip, group, coarse, zc, uc)
            else:
                assert zc is None and uc is None
            z_only = _ok(hip, group, fine, coarse if with_coarse else None, ld_in=n + pad_in, ld_out=n + pad_out, want_u=False)
            assert _bits(z_only[0], zf) and (not with_coarse or _bits(z_only[1], zc))


def test_every_instance_of_the_kernel(hip):
    """601 effective coefficients (more than the 512 that LDS holds: coefficients and row from global memory), few coefficients on
    a rule of 4100 cells (the row does not fit into LDS with them), and both beside the all-LDS instance: u bit for bit the CDF entry's"""
    import mlmc_amd
    from mlmc_amd.tool import simple_distribution as sd
    rng = np.random.default_rng(3)
    dom = (-4.0, 6.0)
    size, K = 601, 25
    matrix = np.zeros((K, size))
    matrix[np.arange(K), np.arange(K)] = 1.0
    matrix[1, 600] = 0.125                               # the last coefficient is in use
    fn = mlmc_amd.TransformedMoments(mlmc_amd.Fourier(size, dom), matrix)
    lam = np.zeros(K)
    lam[:5] = [np.log(10.0), 0.7, -0.4, 0.2, 0.1]
    lam[24] = 0.05

    def big(quad):
        d = sd.SimpleDistribution(fn, np.stack([np.eye(K)[0], np.ones(K)], axis=1), domain=dom)
        d.multipliers, d._moment_errs = lam.copy(), np.ones(K)
        d.n_intervals, d._gauss_degree = quad
        return d
    for quad in ((64, 21), (4100, 3)):
        small = _closed(5.0, (0.5, 4.5), quad)
        for distrs in ([big(quad), small, big(quad)], [small, small]):
            x = np.array([d.domain[0] + (d.domain[1] - d.domain[0]) * rng.random(257) for d in distrs])
            c = np.array([d.domain[0] + (d.domain[1] - d.domain[0]) * rng.random(257) for d in distrs])
            c[0, 5] = np.nan
            zf, zc, uf, uc = sd.normal_scores(distrs, x, c, return_uniforms=True)
            want_f, want_c = sd.cdfs_on_rule(distrs, list(x)), sd.cdfs_on_rule(distrs, list(c))
            assert _bits(uf, np.array(want_f)) and np.all(np.isfinite(zf))
            keep = np.isfinite(c)
            assert _bits(uc[keep], np.array(want_c)[keep]) and np.isnan(uc[0, 5]) and np.isnan(zc[0, 5]) and np.all(np.isfinite(zc[keep]))
            alone = sd.normal_scores(distrs, x)
            assert _bits(alone, zf)


def test_scores_against_mpmath(hip, table):
    """z against mpmath's Phi^-1 (50 digits) of the device's own clamped u, in units of 2^-53 max(1, |z|): 2004 points of the six
    cases, fine and coarse, the ends of the clamp among them"""
    rng = np.random.default_rng(17)
    group = table[0]
    n = 167
    fine, coarse = _points(rng, group, n, outside=False), _points(rng, group, n, outside=False)
    for m, p in enumerate(group):
        a, b = p["dist"].domain
        fine[m, 0], coarse[m, 0] = np.nextafter(a, b), np.nextafter(b, a)
    zf, zc, uf, uc = _ok(hip, group, fine, coarse)
    z, u = np.concatenate([zf.ravel(), zc.ravel()]), np.concatenate([uf.ravel(), uc.ravel()])
    assert z.size == 2004 and np.all(np.isfinite(z)) and np.all((u >= 0.0) & (u <= 1.0))
    clamped = np.minimum(np.maximum(u, sk.U_LO), sk.U_HI)
    assert z.min() < -5.0 and z.max() > 5.0                                              # both tails
    units = jc.z_units(z, jc.mp_ndtri(clamped))
    k = int(np.argmax(units))
    print(f"\nnormcdfinv on the device at arbitrary doubles: worst {units[k]:.4g} units at u = {clamped[k]!r} (recorded "
          f"{sk.Z_UNITS_OBSERVED}, tolerance {sk.z_tolerance():g})")
    assert units[k] <= sk.z_tolerance()


@pytest.mark.parametrize("quad", qc.RULES)
def test_closed_forms(hip, quad):
    """z == ndtri(F(x)) for the truncated exponentials and the uniform: within the normcdfinv tolerance plus the CDF tolerance of
    the quantile tests (units of 2^-53 F(x)) carried through Phi^-1, |dz| = |du| / phi(z)"""
    from mlmc_amd.tool import simple_distribution as sd
    rng = np.random.default_rng(23)
    distrs = _closed_three(quad)
    group = [dict(domain=d) for d in sk.DOMAINS]
    x = _points(rng, group, 1000, outside=False)
    z, u = sd.normal_scores(distrs, x, return_uniforms=True)
    cdf_units = mc.device_tolerance(mc.cases()["mix_R9"], "integral")
    worst = 0.0
    for m, (rate, dom) in enumerate(zip(sk.RATES, sk.DOMAINS)):
        F = sk.closed_cdf(rate, dom, x[m])
        ref = special.ndtri(F)
        phi = np.exp(-0.5 * ref * ref) / np.sqrt(2 * np.pi)
        assert np.all(np.abs(u[m] - F) <= cdf_units * U * F)
        bound = sk.z_tolerance() * U * np.maximum(1.0, np.abs(ref)) + cdf_units * U * F / phi + 16 * U * np.maximum(1.0, np.abs(ref))
        worst = max(worst, float(np.max(np.abs(z[m] - ref) / bound)))
        assert np.all(np.abs(z[m] - ref) <= bound), (rate, dom)
    print(f"\nclosed forms on {quad}: worst error / bound {worst:.3g}")


def test_specials(hip, table):
    """a row holding NaN, +-inf, a, b, nextafter inside and outside both ends and a value far outside: exactly the strictly-inside
    ones are finite.  A NaN-mass problem and a NaN-coefficient problem among valid ones: their rows are NaN, the others untouched"""
    group = list(table[0][:5])
    M = len(group)
    inside = np.array([False, False, False, False, False, True, False, True, False, False, True])
    x = np.empty((M, inside.size))
    for m, p in enumerate(group):
        a, b = p["dist"].domain
        x[m] = [np.nan, -np.inf, np.inf, a, b, np.nextafter(a, b), np.nextafter(a, -np.inf), np.nextafter(b, a), np.nextafter(b, np.inf),
                b + 1e6 * (b - a), 0.5 * (a + b)]
    for coarse in (None, x[:, ::-1].copy()):
        zf, zc, uf, uc = _ok(hip, group, x, coarse)
        for z, u, mask in ((zf, uf, inside), (zc, uc, inside[::-1])):
            if z is None:
                continue
            assert np.array_equal(np.isfinite(z), np.tile(mask, (M, 1))) and np.array_equal(np.isfinite(u), np.tile(mask, (M, 1)))
            assert np.all(np.isnan(z[:, ~mask])) and np.all(np.isnan(u[:, ~mask]))
            assert np.all((u[:, mask] >= 0.0) & (u[:, mask] <= 1.0)) and np.all(np.abs(z[:, mask]) <= 8.3)
    # degenerate problems: NaN multipliers (all, and the last one alone), and a domain that reaches outside the domain of the moments
    rng = np.random.default_rng(29)
    pts = _points(rng, group, 257)
    coarse = _points(rng, group, 257)
    want = _ok(hip, group, pts, coarse, want_mass=True)
    bad = dict(group[1])
    bad["lam"] = np.full_like(group[1]["lam"], np.nan)
    one_nan = dict(group[3])
    one_nan["lam"] = group[3]["lam"].copy()
    one_nan["lam"][-1] = np.nan
    doms = [p["dist"].domain for p in group]
    wide = list(doms)
    wide[4] = (doms[4][0] - 1.0, doms[4][1])
    got = _ok(hip, [group[0], bad, group[2], one_nan, group[4]], pts, coarse, want_mass=True, domains=wide)
    for g, w in zip(got[:4], want[:4]):
        assert np.all(np.isnan(g[[1, 3, 4]])) and _bits(g[[0, 2]], w[[0, 2]])
    assert got[4][0] == want[4][0] and got[4][2] == want[4][2] and not np.isfinite(got[4][4])


def test_independence(hip, table):
    """an element's bits do not change with M, the row's position, n, ld_in / ld_out, the presence of coarse, or a second run"""
    rng = np.random.default_rng(31)
    group = _cycle(table[1], 65)
    fine, coarse = _points(rng, group, 1000), _points(rng, group, 1000)
    zf, zc, uf, uc = _ok(hip, group, fine, coarse)
    again = _ok(hip, group, fine, coarse, ld_in=1003, ld_out=1007)
    assert all(_bits(a, w) for a, w in zip(again, (zf, zc, uf, uc)))
    no_coarse = _ok(hip, group, fine)
    assert _bits(no_coarse[0], zf) and _bits(no_coarse[2], uf)
    swapped = _ok(hip, group, coarse, fine)
    assert _bits(swapped[0], zc) and _bits(swapped[1], zf)
    as_fine = _ok(hip, group, coarse)
    assert _bits(as_fine[0], zc)
    for m in (0, 16, 63, 64):
        alone = _ok(hip, [group[m]], fine[m:m + 1], coarse[m:m + 1])
        assert _bits(alone[0][0], zf[m]) and _bits(alone[1][0], zc[m]) and _bits(alone[2][0], uf[m]), m
    sub = _ok(hip, group[3:20], fine[3:20], coarse[3:20])
    assert _bits(sub[0], zf[3:20]) and _bits(sub[1], zc[3:20])
    rev = _ok(hip, group[::-1], fine[::-1], coarse[::-1])
    assert _bits(rev[0], zf[::-1]) and _bits(rev[1], zc[::-1])
    for lo, hi in ((50, 150), (0, 1), (255, 257), (489, 1000)):
        part = _ok(hip, group, fine[:, lo:hi], coarse[:, lo:hi])
        assert _bits(part[0], zf[:, lo:hi]) and _bits(part[1], zc[:, lo:hi])
        part = _ok(hip, group, fine[:, lo:hi])
        assert _bits(part[0], zf[:, lo:hi])


def test_normal_scores_python(hip, table):
    """normal_scores == the C entry; host and device input, device output; one upload"""
    import torch
    from mlmc_amd.tool import simple_distribution as sd
    rng = np.random.default_rng(37)
    group = table[1][:3]
    distrs = [p["dist"] for p in group]
    fine, coarse = _points(rng, group, 257), _points(rng, group, 257)
    zf, zc, uf, uc = _ok(hip, group, fine, coarse)
    got = sd.normal_scores(distrs, fine, coarse, return_uniforms=True)
    assert all(isinstance(g, np.ndarray) and _bits(g, w) for g, w in zip(got, (zf, zc, uf, uc)))
    assert _bits(sd.normal_scores(distrs, fine), zf)
    pair = sd.normal_scores(distrs, fine, coarse)
    assert len(pair) == 2 and _bits(pair[0], zf) and _bits(pair[1], zc)
    z1, u1 = sd.normal_scores(distrs, fine, return_uniforms=True)
    assert _bits(z1, zf) and _bits(u1, uf)
    on_dev = sd.normal_scores(distrs, torch.from_numpy(fine).cuda(), torch.from_numpy(coarse).cuda(), device=True)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 for t in on_dev)
    assert _bits(on_dev[0].cpu().numpy(), zf) and _bits(on_dev[1].cpu().numpy(), zc)
    assert sd.normal_scores(distrs, np.zeros((3, 0))).shape == (3, 0)
    mixed = [distrs[0], table[0][1]["dist"], distrs[2]]
    with pytest.raises(ValueError, match="same quadrature"):
        sd.normal_scores(mixed, fine)


def test_round_trip(hip, table):
    """quantiles(Phi(z)) returns x: in terms of the long-double Fhat, |Fhat(x') - Fhat(x)| stays within the quantile tolerance at
    p = Phi(z) plus what the score itself may be off by (the CDF tolerance, the normcdfinv tolerance through phi, the rounding of Phi)"""
    from mlmc_amd.tool import simple_distribution as sd
    rng = np.random.default_rng(41)
    group = table[0]
    distrs = [p["dist"] for p in group]
    # values where the mass is: the quantiles of probabilities in (0.001, 0.999), so that no score sits at the clamp
    x = np.array(sd.quantiles(distrs, [0.001 + 0.998 * rng.random(100) for _ in group]))
    z = sd.normal_scores(distrs, x)
    p = special.ndtr(z)
    back = sd.quantiles(distrs, list(p))
    worst = 0.0
    for pr, xr, zr, pp, xb in zip(group, x, z, p, back):
        case = pr["case"]
        ref = qc.RuleTable(case, pr["lam"], pr["quad"])
        F0, s0 = ref.fhat(xr)
        F1, s1 = ref.fhat(xb)
        phi = np.exp(-0.5 * zr * zr) / np.sqrt(2 * np.pi)
        bound = (LD(qc.quantile_tolerance(case)) * U * (s1 + pp) + 4 * ref.density(xb) * np.spacing(np.abs(xb)).astype(LD) / ref.T
                 + LD(mc.device_tolerance(case, "integral")) * U * s0 + phi * sk.z_tolerance() * U * np.maximum(1.0, np.abs(zr)) + 8 * U * pp)
        err = np.abs(F1 - F0)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), pr["tag"]
    print(f"\nround trip: worst error / bound {worst:.3g}")


# ---- the estimate -----------------------------------------------------------------------------------------------------------
def _storage(levels):
    """a DeviceMemory storage of a vector quantity with M components from [(fine [M, n], coarse [M, n] | None)]"""
    import torch
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    from mlmc_amd.sample_storage import DeviceMemory
    M = levels[0][0].shape[0]
    steps = [0.5 * 0.2 ** l for l in range(len(levels))]
    spec = [QuantitySpec(name="q", unit="m", shape=(M, 1), times=[1], locations=['0'])]
    dev = DeviceMemory()
    dev.save_global_data(result_format=spec, level_parameters=[[s] for s in steps])
    for l, (f, c) in enumerate(levels):
        c = np.zeros_like(f) if c is None else c
        dev.set_level_samples(l, torch.from_numpy(np.stack([f, c], axis=-1)).cuda())
    return dev, spec


def _estimate(levels):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.quantity.quantity import make_root_quantity
    dev, spec = _storage(levels)
    qe.device_cache_clear()
    q = make_root_quantity(dev, spec)['q']
    return Estimate(q, dev, Legendre(2, (-1.0, 1.0)))


def _densities(distrs):
    return [(d, None, types.SimpleNamespace(success=True), None) for d in distrs]


def _accumulation_levels():
    """3 levels, M = 3, n = (1000, 257, 65) pairs of the closed-form marginals: fine from correlated normals, coarse = fine
    perturbed, with NaN and out-of-domain entries in fine and coarse of different components"""
    rng = np.random.default_rng(43)
    F = np.linalg.cholesky(sk.CORR)
    levels = []
    for l, n in enumerate((1000, 257, 65)):
        y = F @ rng.standard_normal((3, n))
        f = np.array([sk.closed_quantile(r, d, special.ndtr(row)) for r, d, row in zip(sk.RATES, sk.DOMAINS, y)])
        c = None
        if l > 0:
            yc = y + 0.3 * 0.5 ** l * rng.standard_normal((3, n))
            c = np.array([sk.closed_quantile(r, d, special.ndtr(row)) for r, d, row in zip(sk.RATES, sk.DOMAINS, yc)])
            c[0, 2::11] = np.nan
            c[2, 5::13] = sk.DOMAINS[2][1] + 0.5
        f[1, 1::7] = np.nan
        f[0, 3::17] = sk.DOMAINS[0][0]                  # the end point itself drops
        levels.append((f, c))
    return levels


def _score_sums_ld(levels, distrs):
    """long-double level sums of the device's own scores with a row of ones: per level (n, n_rm, s, sp, sa, sq) as the
    component-covariance tests have them (sa / sq: the sums of |f_i f_j| + |c_i c_j| and of its square)"""
    from mlmc_amd.tool import simple_distribution as sd
    out = []
    for f, c in levels:
        got = sd.normal_scores(distrs, f, c, device=True)
        zf, zc = (got, None) if c is None else got
        zf = zf.cpu().numpy()
        zc = None if zc is None else zc.cpu().numpy()
        bad = np.isnan(zf).any(axis=0) | (np.zeros(zf.shape[1], bool) if zc is None else np.isnan(zc).any(axis=0))
        Ff = np.vstack([zf[:, ~bad], np.ones((1, int((~bad).sum())))]).astype(LD)
        Y = np.einsum("ik,jk->kij", Ff, Ff)
        A = np.abs(Y)
        if zc is not None:
            Cc = np.vstack([zc[:, ~bad], np.ones((1, int((~bad).sum())))]).astype(LD)
            Z = np.einsum("ik,jk->kij", Cc, Cc)
            Y = Y - Z
            A = A + np.abs(Z)
        out.append((int((~bad).sum()), int(bad.sum()), Y.sum(axis=0), (Y * Y).sum(axis=0), A.sum(axis=0), (A * A).sum(axis=0)))
    return out


def test_accumulation(hip):
    """estimate_score_correlation == the long-double telescoping sums of the device's own scores.  The bound is the one the
    component-covariance tests apply to the accumulator's level sums, |s - ref| <= 1e-10 max(|ref|, sum of the sizes of the terms)
    (and the same for the sums of squares), carried through mean_l = s_l / n_l, the telescoping sum and cov = E[z z^T] - m m^T;
    the counts are exact.  The column-block size of the Python path changes the sums by no more than that either."""
    from mlmc_amd.quantity import quantity_estimate as qe
    levels = _accumulation_levels()
    distrs = _closed_three()
    M = 3
    est = _estimate(levels)
    res = est.estimate_score_correlation(densities=_densities(distrs))
    ref = _score_sums_ld(levels, distrs)
    n = np.array([r[0] for r in ref])
    assert np.array_equal(res.n_samples, n) and np.array_equal(res.n_rm_samples, [r[1] for r in ref])
    assert res.n_samples.dtype == np.int64 and np.all(n < [1000, 257, 65]) and np.all(n > 30)
    second = sum(r[2] / LD(r[0]) for r in ref)
    b_second = sum(1e-10 * np.maximum(np.abs(r[2]), r[4]) / LD(r[0]) for r in ref)
    mean, b_mean = second[M, :M], b_second[M, :M]
    cov = second[:M, :M] - np.outer(mean, mean)
    b_cov = b_second[:M, :M] + np.outer(np.abs(mean), b_mean) + np.outer(b_mean, np.abs(mean)) + np.outer(b_mean, b_mean) + 4 * U
    var_l = [(r[3] - r[2] * r[2] / LD(r[0])) / LD(r[0] - 1) / LD(r[0]) for r in ref]
    b_var_l = [(1e-10 * np.maximum(np.abs(r[3]), r[5]) + 2 * np.abs(r[2]) * 1e-10 * np.maximum(np.abs(r[2]), r[4]) / LD(r[0]))
               / LD(r[0] - 1) / LD(r[0]) for r in ref]
    cov_var, b_cov_var = sum(var_l)[:M, :M], sum(b_var_l)[:M, :M]

    def check(res):
        assert res.corr.shape == (M, M) and res.cov.shape == (M, M) and res.cov_var.shape == (M, M)
        assert res.mean.shape == (M,) and res.var.shape == (M,)
        assert np.all(np.abs(res.mean - mean) <= b_mean)
        assert np.all(np.abs(res.cov - cov) <= b_cov) and np.array_equal(res.cov, res.cov.T)
        assert np.array_equal(res.var, np.diag(res.cov))
        assert np.all(np.abs(res.cov_var - cov_var) <= b_cov_var + 1e-300)
        sd_ = np.sqrt(np.diag(cov).astype(np.float64))
        want = (cov / sd_[:, None] / sd_[None, :]).astype(np.float64)
        # corr_ij = cov_ij / sqrt(cov_ii cov_jj) with |corr| <= 1: the errors of the three entries add up, relative to the variances
        tol_corr = float(4 * np.max(b_cov) / np.min(np.diag(cov)) + 8 * U)
        assert np.array_equal(np.diag(res.corr), np.ones(M)) and np.max(np.abs(res.corr - want)[~np.eye(M, dtype=bool)]) <= tol_corr
    check(res)
    print(f"\naccumulation: mean {res.mean}, var {res.var}, kept {res.n_samples}, dropped {res.n_rm_samples}")
    again = est.estimate_score_correlation(densities=_densities(distrs))
    assert all(np.array_equal(a, b) for a, b in zip(again, res))                         # the same input gives the same bits
    assert "MLMC_SCORE_BLOCK_COLUMNS" not in os.environ
    os.environ["MLMC_SCORE_BLOCK_COLUMNS"] = "96"        # blocks of 96 columns: 11 for level 0, 96 + 96 + 65 for level 1, one for level 2
    try:
        assert qe.score_block_columns(M) == 96
        blocks = est.estimate_score_correlation(densities=_densities(distrs))
    finally:
        del os.environ["MLMC_SCORE_BLOCK_COLUMNS"]
    assert np.array_equal(blocks.n_samples, res.n_samples) and np.array_equal(blocks.n_rm_samples, res.n_rm_samples)
    check(blocks)
    # without scores nothing changes: the plain covariance of the same storage
    cov_plain, _ = est.estimate_component_covariance()
    assert cov_plain.shape == (M, M) and np.all(np.isfinite(cov_plain))
    bad = _densities(_closed_three())
    bad[1][0].multipliers = np.array([np.nan, np.nan])
    with pytest.raises(Exception, match="All samples were masked|component 1"):
        est.estimate_score_correlation(densities=bad)


@pytest.mark.parametrize("first", sk.FIRSTS)
def test_copula_case_end_to_end(hip, first):
    """draws of joint_samples with the known factor in a one-level storage: the score correlation is within 5 standard errors of the
    latent one, the Pearson correlation that sample_joint(corr=None) uses is more than 20 away for the (5, -5) pair, and
    sample_joint(corr="scores") uses correlation_factor(estimate_score_correlation().corr)"""
    from mlmc_amd.tool import simple_distribution as sd
    distrs = _closed_three()
    pdfs = _densities(distrs)
    F, _ = sd.correlation_factor(sk.CORR)
    x = sd.joint_samples(distrs, sk.N_COPULA, sk.SEED, factor=F, first=first)
    est = _estimate([(x, None)])
    res = est.estimate_score_correlation(densities=pdfs)
    n = int(res.n_samples[0])
    assert n + int(res.n_rm_samples[0]) == sk.N_COPULA and n >= sk.N_COPULA - 4
    score_err = sk.correlation_errors(res.corr, sk.CORR, n)
    _, _, used_pearson = est.sample_joint(16, sk.SEED + 1, densities=pdfs)
    pearson_err = sk.correlation_errors(used_pearson, sk.CORR, n)
    print(f"\nfirst = {first}: score correlation {score_err.max():.3g} standard errors; Pearson of the (5, -5) pair "
          f"{used_pearson[0, 1]:.4f}, {pearson_err[0]:.3g} standard errors from 0.8; score mean {res.mean}, var {res.var}")
    assert score_err.max() <= 5.0
    assert pearson_err[0] > 20.0
    # calibration: mean 0 and variance 1 of every component's scores, within 6 standard errors of a standard normal sample
    assert np.all(np.abs(res.mean) <= 6.0 / np.sqrt(n)) and np.all(np.abs(res.var - 1.0) <= 6.0 * np.sqrt(2.0 / n))
    draws, ok, used = est.sample_joint(64, sk.SEED + 1, corr="scores", densities=pdfs)
    Fs, _ = sd.correlation_factor(res.corr)
    assert np.array_equal(used, Fs @ Fs.T) and draws.shape == (3, 64) and np.all(ok)
    assert _same(draws, sd.joint_samples(distrs, 64, sk.SEED + 1, factor=Fs))


def test_errors_and_no_ops(hip, table):
    import torch
    group = _cycle(table[0], 4)
    rng = np.random.default_rng(47)
    fine, coarse = _points(rng, group, 8), _points(rng, group, 8)

    def expect(rc, pattern):
        with pytest.raises(hip.MlmcHipError, match=pattern):
            hip.check(rc)
    assert _scores(hip, group, fine, coarse)[0] == 0
    expect(_raw(hip, group, n=8, ld_in=7), NAME + ": ld_in and ld_out")
    expect(_raw(hip, group, n=8, ld_out=7), NAME + ": ld_in and ld_out")
    expect(_raw(hip, group, n=-1), NAME + ": n < 0")
    expect(_raw(hip, group, M=-1), NAME + ": M < 0")
    expect(_raw(hip, group, fine=None), NAME + ": null argument")
    expect(_raw(hip, group, z_fine=None), NAME + ": null argument")
    expect(_raw(hip, group, z_coarse=None), NAME + ": null argument")
    expect(_raw(hip, group, quad=(-1, 21)), NAME + ".*n_intervals")
    expect(_raw(hip, group, quad=(64, 65)), NAME + ".*gauss_degree")
    # aliasing: an output on an input, an output inside an input's rows, two outputs on each other
    expect(_raw(hip, group, z_fine="fine"), NAME + ": an output array overlaps an input array")
    expect(_raw(hip, group, z_coarse="fine"), NAME + ": an output array overlaps an input array")
    expect(_raw(hip, group, u_fine="coarse"), NAME + ": an output array overlaps an input array")
    expect(_raw(hip, group, u_coarse="coarse+3"), NAME + ": an output array overlaps an input array")
    expect(_raw(hip, group, z_coarse="z_fine"), NAME + ": two output arrays overlap")
    expect(_raw(hip, group, u_fine="z_fine+1"), NAME + ": two output arrays overlap")
    assert _raw(hip, group, coarse=None, z_coarse="fine") == 0                           # without coarse z_coarse is ignored
    null_h = (C.c_void_p * 4)(*[_fn(p["case"])._basis_handle().value for p in group])
    null_h[2] = None
    expect(_raw(hip, group, handles=null_h), NAME + ": problem 2.*null basis")
    expect(_raw(hip, group, bad_domain=3), NAME + ": problem 3.*domain")
    # no-ops: M = 0, and n = 0 (the arrays may be NULL then and are not touched; the masses are still returned)
    assert hip.lib().mlmc_density_scores_batch(0, None, None, None, None, None, None, 0, 0, None, None, 5, 5, None, None, 5, None, None,
                                               None) == 0
    assert _raw(hip, group, n=0) == 0 and _raw(hip, group, n=0, fine=None, coarse=None, z_fine=None, z_coarse=None) == 0
    mass = np.full(4, -1.0)
    assert _raw(hip, group, n=0, fine=None, coarse=None, z_fine=None, z_coarse=None, mass=mass) == 0
    assert np.array_equal(mass, _cdf(hip, group, np.zeros((4, 0)))[1]) and np.all(mass > 0)
    torch.cuda.synchronize()


def _raw(hip, group, M=4, n=8, ld_in=8, ld_out=8, fine="own", coarse="own", z_fine="own", z_coarse="own", u_fine=None, u_coarse=None,
         quad=None, handles=None, bad_domain=None, mass=None):
    """the raw entry on arrays of in-domain values; an array argument is "own" (a fresh device array), None, or the name of another
    argument with an optional +offset in doubles (aliasing)"""
    import torch
    h, r1, lam, sig, a, b = _problem_args(hip, group)
    if bad_domain is not None:
        b = b.copy()
        b[bad_domain] = a[bad_domain]
    mid = torch.from_numpy(np.tile(0.5 * (a + b)[:, None], (1, max(ld_in, ld_out, 8)))).cuda().contiguous()
    arrays = {}

    def resolve(name, spec):
        if spec is None:
            return None
        if spec == "own":
            arrays[name] = mid.clone()
            return arrays[name].data_ptr()
        base, _, off = spec.partition("+")
        return arrays[base].data_ptr() + 8 * int(off or 0)
    ptrs = {}
    for name, spec in (("fine", fine), ("coarse", coarse), ("z_fine", z_fine), ("z_coarse", z_coarse), ("u_fine", u_fine),
                       ("u_coarse", u_coarse)):
        ptrs[name] = resolve(name, spec)
    torch.cuda.synchronize()
    quad = group[0]["quad"] if quad is None else quad
    P = C.c_void_p
    rc = hip.lib().mlmc_density_scores_batch(M, C.cast(h if handles is None else handles, C.c_void_p), hip.ptr(r1), hip.ptr(lam), hip.ptr(sig),
                                             hip.ptr(a), hip.ptr(b), quad[0], quad[1], P(ptrs["fine"]), P(ptrs["coarse"]), n, ld_in,
                                             P(ptrs["z_fine"]), P(ptrs["z_coarse"]), ld_out, P(ptrs["u_fine"]), P(ptrs["u_coarse"]),
                                             hip.ptr(mass))
    torch.cuda.synchronize()
    return rc


def test_kernel_time_counts_the_scores_kernel(hip, table):
    group = table[0]
    rng = np.random.default_rng(53)
    ms, launches = C.c_double(), C.c_int64()
    hip.check(hip.lib().mlmc_density_quantiles_kernel_time(C.byref(ms), C.byref(launches)))
    _ok(hip, group, _points(rng, group, 1000), _points(rng, group, 1000))
    hip.check(hip.lib().mlmc_density_quantiles_kernel_time(C.byref(ms), C.byref(launches)))
    assert launches.value == 1 and ms.value > 0
