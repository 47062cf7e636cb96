"""GPU tests of the joint sampling through a Gaussian copula (k_cop_normals / k_cop_uniforms in mlmc_amd/csrc/copula.hip and the
U_IN instances of k_q_sample in density.hip) through mlmc_density_sample_joint_batch, simple_distribution.joint_samples and
Estimate.sample_joint.

x[m][j] = Q_m(u[m][j]), u = clamp(Phi(F z)) (include/mlmc_hip.h).  The normals are compared with mpmath at the NumPy restatement of
their uniforms (tests/joint_sample_cases.py), Phi with mpmath at the device's own normals, the matrix product with a long-double dot
of the device's normals, the structure of the product and the inversion bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy import special

from tests import joint_sample_cases as jc
from tests import maxent_cases as mc
from tests import quantile_cases as qc
from tests import sample_cases as sc
from tests.test_gpu_density_samples import CASES, FAR, SEED, _quantiles_c, _same, _small_vector_storage
from tests.test_gpu_quantiles import _dist, _fn, _raw_args

pytestmark = pytest.mark.gpu
NAME = "mlmc_density_sample_joint_batch"
U = jc.U


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


def _joint(hip, group, F, n, seed=SEED, streams=None, first=0, flags=0, kind=None, want_u=True, want_z=True, want_mass=False):
    """mlmc_density_sample_joint_batch on the problems of `group`; returns (rc, out [M, n], u [M, n], z [K, n], mass)"""
    import torch
    kind = hip.HOST if kind is None else kind
    M = len(group)
    F = np.ascontiguousarray(F, dtype=np.float64)
    K = F.shape[1]
    handles, r1, lam, sig = _raw_args(hip, group)
    a = np.array([p["case"].domain[0] for p in group], dtype=np.float64)
    b = np.array([p["case"].domain[1] for p in group], dtype=np.float64)
    st = None if streams is None else np.ascontiguousarray(streams, dtype=np.uint32)
    cols = max(int(n), 0)

    def array(rows, want):
        if not want:
            return None
        if kind == hip.DEVICE:
            return torch.full((rows, cols), 7.25, dtype=torch.float64, device="cuda")
        return np.full((rows, cols), 7.25)
    out, u, z = array(M, True), array(M, want_u), array(K, want_z)
    if kind == hip.DEVICE:
        torch.cuda.synchronize()
    mass = np.full(M, -1.0) if want_mass else None
    quad = group[0]["quad"]
    rc = hip.lib().mlmc_density_sample_joint_batch(M, C.cast(handles, C.c_void_p), hip.ptr(r1), hip.ptr(lam), hip.ptr(sig), hip.ptr(a),
                                                   hip.ptr(b), quad[0], quad[1], K, hip.ptr(F), seed, hip.ptr(st), first, n, flags,
                                                   hip.ptr(out), hip.ptr(u), hip.ptr(z), hip.ptr(mass), kind)
    if kind == hip.DEVICE:
        out, u, z = (None if v is None else v.cpu().numpy() for v in (out, u, z))
    return rc, out, u, z, mass


def _ok(hip, *args, **kw):
    rc, out, u, z, mass = _joint(hip, *args, **kw)
    hip.check(rc)
    return out, u, z, mass


STREAMS5 = [0, 7, 2 ** 32 - 1, 11, 3]


@pytest.fixture(scope="module")
def identity(hip, table):
    """F = I, M = K = 5, 400 draws from first = 2^33 + 1 under explicit streams: 2000 normals and, y = z exactly, Phi alone"""
    out, u, z, _ = _ok(hip, _cycle(table[0], 5), np.eye(5), 400, streams=STREAMS5, first=FAR)
    return u, z


def test_normals(hip, table, identity):
    """z_out against mpmath at the bit-exact NumPy uniforms, in units of 2^-53 max(1, |z|); the antithetic pairs are exact"""
    _, z = identity
    u0, _ = jc.latent_uniforms(SEED, STREAMS5, FAR, 400)
    assert z.shape == (5, 400) and np.all(np.isfinite(z)) and z.min() < -2.5 and z.max() > 2.5       # both tails
    units = jc.z_units(z, jc.mp_ndtri(u0))
    k = int(np.argmax(units))
    print(f"\nnormcdfinv on the device: worst {units[k]:.4g} units at u0 = {u0.ravel()[k]!r} (recorded {jc.Z_UNITS_OBSERVED}, "
          f"tolerance {jc.z_tolerance():g})")
    assert units[k] <= jc.z_tolerance()
    group = _cycle(table[0], 2)
    F = jc.random_factor(np.random.default_rng(1), 2, 3)
    for first in (6, FAR + 1):
        _, _, both, _ = _ok(hip, group, F, 21, first=first, flags=1)
        _, _, plain, _ = _ok(hip, group, F, 12, first=first // 2)
        j = first + np.arange(21)
        even, odd = both[:, j % 2 == 0], both[:, j % 2 == 1]
        assert _same(even, plain[:, (j[j % 2 == 0] // 2) - first // 2])
        assert _same(odd, -plain[:, (j[j % 2 == 1] // 2) - first // 2])
    _, _, both, _ = _ok(hip, group, F, 1000, flags=1)
    assert np.array_equal(both[:, 1::2], -both[:, ::2]) and _same(both[:, ::2], _ok(hip, group, F, 500)[2])


def test_normcdf_alone(hip, identity):
    """F = I: y = z exactly, so u_out == clamp(Phi(z_out)) against mpmath, in units of 2^-53 max(Phi, 2^-53)"""
    u, z = identity
    units = jc.phi_units(u, jc.mp_ncdf(z))
    k = int(np.argmax(units))
    print(f"\nnormcdf on the device: worst {units[k]:.4g} units at z = {z.ravel()[k]!r} (recorded {jc.PHI_UNITS_OBSERVED}, "
          f"tolerance {jc.phi_tolerance():g})")
    assert units[k] <= jc.phi_tolerance()
    assert np.all((u >= jc.U_LO) & (u <= jc.U_HI))


@pytest.mark.parametrize("M,K,n,first", [(1, 1, 17, 0), (2, 4, 255, 3), (3, 3, 1000, 0), (16, 17, 64, FAR), (17, 5, 257, 3), (65, 65, 65, 0)])
def test_gemm_and_epilogue(hip, table, M, K, n, first):
    """random row-normalised F: u_out against Phi of the long-double dot of F with the device's own z_out, within the first-order
    bound of the dot product, phi(y) (K + 2) 2^-53 sum_k |F_mk z_k|, plus the normcdf error E_Phi"""
    F = jc.random_factor(np.random.default_rng(100 * M + K), M, K)
    _, u, z, _ = _ok(hip, _cycle(table[1], M), F, n, first=first)
    y = jc.ld_dot(F, z)
    phi = jc.mp_ncdf(y)
    ref = np.array([float(v) for v in phi]).reshape(M, n)
    err = jc.phi_abs_errors(u, phi).reshape(M, n)
    yd = y.astype(np.float64)
    dens = np.exp(-0.5 * yd * yd) / np.sqrt(2 * np.pi)
    bound = dens * (K + 2) * U * (np.abs(F) @ np.abs(z)) + jc.phi_tolerance() * U * np.maximum(ref, U)
    k = int(np.argmax(err / bound))
    print(f"\nM {M} K {K} n {n}: worst error / bound {(err / bound).ravel()[k]:.3g}")
    assert np.all(err <= bound)


def test_exact_structure(hip, table):
    """rows of F with a single 1, a permutation, equal rows, ones [M, 1], [[1], [-1]]"""
    rng = np.random.default_rng(5)
    group = _cycle(table[0], 65)
    _, ident, z_id, _ = _ok(hip, group, np.eye(65), 65)
    perm = rng.permutation(65)
    _, u, z, _ = _ok(hip, group, np.eye(65)[perm], 65)
    assert _same(u, ident[perm]) and _same(z, z_id)
    # 17 rows picking columns of 65 latent normals, with repeats: each row is the F = I row of its column, equal rows are equal
    cols = np.array([64, 0, 33, 64, 15, 16, 17, 31, 32, 33, 47, 48, 63, 1, 0, 64, 5])
    pick = np.zeros((17, 65))
    pick[np.arange(17), cols] = 1.0
    _, u, _, _ = _ok(hip, group[:17], pick, 65)
    assert _same(u, ident[cols]) and _same(u[0], u[3]) and _same(u[1], u[14])
    # and the other way round: 65 rows on 4 latent normals, rows in both row tiles
    cols = rng.integers(0, 4, 65)
    pick = np.zeros((65, 4))
    pick[np.arange(65), cols] = 1.0
    _, u, _, _ = _ok(hip, group, pick, 257)
    _, ident4, _, _ = _ok(hip, group[:4], np.eye(4), 257)
    assert _same(u, ident4[cols])
    # equal general rows
    F = jc.random_factor(rng, 3, 5)[[0, 1, 0, 2, 1] + [0] * 12]
    _, u, _, _ = _ok(hip, group[:17], F, 63)
    assert _same(u[2], u[0]) and _same(u[4], u[1]) and _same(u[5:], np.tile(u[0], (12, 1))) and not _same(u[0], u[1])
    # comonotone draws of identical distributions
    out, u, _, _ = _ok(hip, [group[0]] * 17, np.ones((17, 1)), 255)
    assert _same(u, np.tile(u[0], (17, 1))) and _same(out, np.tile(out[0], (17, 1))) and len(np.unique(out[0])) == 255
    # countermonotone: u[1] = 1 - u[0] up to the error of two normcdf values and the rounding of the difference
    _, u, _, _ = _ok(hip, group[:2], np.array([[1.0], [-1.0]]), 1000)
    assert np.all(np.abs(u[1] - (1.0 - u[0])) <= 1.01 * jc.phi_tolerance() * U * (u[0] + u[1]) + U)


def test_inversion(hip, table):
    """out == mlmc_density_quantiles_batch(u_out) bit for bit and the masses are equal; host and device arrays, with and without
    u_out / z_out"""
    rng = np.random.default_rng(9)
    for group6 in table:
        quad = group6[0]["quad"]
        for M, K, n, first in ((17, 5, 255, 3), (3, 3, 1000, 0), (65, 4, 63, FAR), (1, 1, 1, 0), (2, 3, 15, 0), (16, 17, 16, 0)):
            group = _cycle(group6, M)
            F = jc.random_factor(rng, M, K)
            out, u, z, mass = _ok(hip, group, F, n, first=first, want_mass=True)
            want, want_mass = _quantiles_c(hip, group, quad, u.ravel(), [n] * M)
            assert _same(out.ravel(), want) and np.array_equal(mass, want_mass), (quad, M, K, n)
            assert np.all(np.isfinite(out)) and np.all(mass > 0)
            for p, row in zip(group, out):
                assert np.all((row >= p["case"].domain[0]) & (row <= p["case"].domain[1]))
            out_d, u_d, z_d, _ = _ok(hip, group, F, n, first=first, kind=hip.DEVICE)
            assert _same(out_d, out) and _same(u_d, u) and _same(z_d, z), (quad, M, K, n)
            for kind in (hip.HOST, hip.DEVICE):
                for want_u, want_z in ((False, False), (True, False), (False, True)):
                    o, uu, zz, _ = _ok(hip, group, F, n, first=first, kind=kind, want_u=want_u, want_z=want_z)
                    assert _same(o, out) and (uu is None or _same(uu, u)) and (zz is None or _same(zz, z)), (quad, M, K, n, kind)


def test_independence(hip, table):
    """first = 50, n = 100 == [50, 150) of n = 150; a row alone == the row in an M = 65 call; the block length of the draws, explicit
    streams that coincide with the default; different seeds differ"""
    rng = np.random.default_rng(11)
    group = _cycle(table[1], 65)
    F = jc.random_factor(rng, 65, 5)
    whole = _ok(hip, group, F, 150)[:3]
    again = _ok(hip, group, F, 150)[:3]
    part = _ok(hip, group, F, 100, first=50)[:3]
    for w, a, p in zip(whole, again, part):
        assert _same(a, w) and _same(p, w[:, 50:])
    for m in (0, 16, 63, 64):
        alone = _ok(hip, [group[m]], F[m:m + 1], 150)
        assert _same(alone[0][0], whole[0][m]) and _same(alone[1][0], whole[1][m]) and _same(alone[2], whole[2]), m
    sub = _ok(hip, group[3:20], F[3:20], 150)
    assert _same(sub[0], whole[0][3:20]) and _same(sub[1], whole[1][3:20])
    explicit = _ok(hip, group, F, 150, streams=np.arange(5))[:3]
    other = _ok(hip, group, F, 150, streams=[0, 1, 2, 3, 9])[:3]
    seed2 = _ok(hip, group, F, 150, seed=SEED + 1)[:3]
    assert all(_same(e, w) for e, w in zip(explicit, whole))
    assert _same(other[2][:4], whole[2][:4]) and not _same(other[2][4], whole[2][4]) and not _same(other[1], whole[1])
    assert not _same(seed2[2], whole[2]) and not _same(seed2[0], whole[0])
    # block seams: 257 draws in blocks of 96 (96 + 96 + 65), host and device arrays, with and without the optional outputs
    F = jc.random_factor(rng, 17, 17)
    want = _ok(hip, group[:17], F, 257, first=3)[:3]
    assert "MLMC_JOINT_BLOCK_DRAWS" not in os.environ
    os.environ["MLMC_JOINT_BLOCK_DRAWS"] = "96"
    try:
        for kind in (hip.HOST, hip.DEVICE):
            got = _ok(hip, group[:17], F, 257, first=3, kind=kind)[:3]
            assert all(_same(g, w) for g, w in zip(got, want)), kind
            assert _same(_ok(hip, group[:17], F, 257, first=3, kind=kind, want_u=False, want_z=False)[0], want[0]), kind
        ms, launches = C.c_double(), C.c_int64()
        hip.check(hip.lib().mlmc_density_quantiles_kernel_time(C.byref(ms), C.byref(launches)))
        _ok(hip, group[:17], F, 257)
        hip.check(hip.lib().mlmc_density_quantiles_kernel_time(C.byref(ms), C.byref(launches)))
        assert launches.value == 3 and ms.value > 0              # one per block
    finally:
        del os.environ["MLMC_JOINT_BLOCK_DRAWS"]
    _ok(hip, group[:17], F, 257)
    hip.check(hip.lib().mlmc_density_quantiles_kernel_time(C.byref(ms), C.byref(launches)))
    assert launches.value == 1


@pytest.mark.parametrize("first", [0, FAR])
def test_statistics_of_the_device_draws(hip, table, first):
    """the 3 x 3 case at n = 16384: the correlations of ndtri(u_out) within 5 standard errors of corr, every row of u_out within the
    DKW bound of uniform, every row of out within it of the long-double Fhat"""
    from mlmc_amd.tool import simple_distribution as sd
    group = table[0][:3]
    F, _ = sd.correlation_factor(jc.CORR3)
    out, u, _, _ = _ok(hip, group, F, sc.DKW_N, first=first)
    errs = jc.correlation_errors(special.ndtri(u), jc.CORR3)
    d_u = [sc.kolmogorov_distance(row) for row in u]
    d_x = [sc.kolmogorov_distance(qc.RuleTable(p["case"], p["lam"], p["quad"]).fhat(row)[0]) for p, row in zip(group, out)]
    print(f"\nfirst = {first}: correlations {errs.max():.3g} standard errors, Kolmogorov distances u {max(d_u):.4f} x {max(d_x):.4f} "
          f"(bound {sc.DKW_BOUND:.5f})")
    assert errs.max() <= 5.0
    assert max(d_u) <= sc.DKW_BOUND and max(d_x) <= sc.DKW_BOUND


def test_degenerate_problem(hip, table):
    """NaN multipliers in one problem among valid ones: its row is NaN, its u_out and every z_out are still written, the other rows
    are bit-equal to a call without it; no error"""
    group = _cycle(table[0], 5)
    bad = dict(group[2])
    bad["lam"] = np.full_like(group[2]["lam"], np.nan)
    F = jc.random_factor(np.random.default_rng(2), 5, 5)
    want, want_u, want_z, want_mass = _ok(hip, group, F, 257, want_mass=True)
    for kind in (hip.HOST, hip.DEVICE):
        out, u, z, mass = _ok(hip, group[:2] + [bad] + group[3:], F, 257, kind=kind, want_mass=True)
        keep = [0, 1, 3, 4]
        assert np.all(np.isnan(out[2])) and _same(out[keep], want[keep]) and _same(u, want_u) and _same(z, want_z)
        assert np.array_equal(mass[keep], want_mass[keep])


def test_errors_and_no_ops(hip, table):
    group = _cycle(table[0], 4)
    F = jc.random_factor(np.random.default_rng(4), 4, 3)

    def expect(rc, pattern):
        with pytest.raises(hip.MlmcHipError, match=pattern):
            hip.check(rc)
    assert _joint(hip, group, F, 2)[0] == 0
    expect(_joint(hip, group, F, -1)[0], NAME + ": n < 0")
    expect(_joint(hip, group, F, 2, first=-1)[0], NAME + ": first < 0")
    expect(_joint(hip, group, F, 2, first=2 ** 63 - 2)[0], NAME + ": first \\+ n overflows")
    assert _joint(hip, group, F, 2, first=2 ** 63 - 3)[0] == 0
    expect(_joint(hip, group, F, 2, kind=5)[0], NAME + ": bad mem_kind")
    expect(_joint(hip, group, F, 2, flags=2)[0], NAME + ": unknown flag")
    expect(_joint(hip, group, F, 2, flags=-1)[0], NAME + ": unknown flag")
    bad = F.copy()
    bad[2] *= 1.0 + 1e-5
    expect(_joint(hip, group, bad, 2)[0], NAME + ": factor row 2.*sum of squares")
    bad = F.copy()
    bad[1] *= 1.0 + 1e-7
    assert _joint(hip, group, bad, 2)[0] == 0
    for value in (np.nan, np.inf):
        bad = F.copy()
        bad[3, 1] = value
        expect(_joint(hip, group, bad, 2)[0], NAME + ": factor row 3.*not finite")
    expect(_joint(hip, group, np.zeros((4, 1)), 2)[0], NAME + ": factor row 0")
    # through the raw entry: K < 1, null arrays, a null basis, a >= b, M < 0
    handles, r1, lam, sig = _raw_args(hip, group)
    a = np.array([p["case"].domain[0] for p in group])
    b = np.array([p["case"].domain[1] for p in group])
    out, quad = np.full((4, 2), 7.25), group[0]["quad"]
    P, lib = hip.ptr, hip.lib()

    def raw(M=4, h=handles, b=b, K=3, F=F, n=2, out=out, mass=None, quad=quad):
        return lib.mlmc_density_sample_joint_batch(M, C.cast(h, C.c_void_p), P(r1), P(lam), P(sig), P(a), P(b), quad[0], quad[1], K, P(F),
                                                   1, None, 0, n, 0, P(out), None, None, P(mass), hip.HOST)
    assert raw() == 0
    expect(raw(K=0), NAME + ": K < 1")
    expect(raw(F=None), NAME + ": null factor")
    expect(raw(out=None), NAME + ".*null")
    expect(raw(M=-1), NAME + ".*M < 0")
    expect(raw(quad=(-1, 21)), NAME + ".*n_intervals")
    expect(raw(quad=(64, 65)), NAME + ".*gauss_degree")
    null_h = (C.c_void_p * 4)(*[_fn(p["case"])._basis_handle().value for p in group])
    null_h[2] = None
    expect(raw(h=null_h), NAME + ": problem 2.*null basis")
    bad_b = b.copy()
    bad_b[3] = a[3]
    expect(raw(b=bad_b), NAME + ": problem 3.*domain")
    # no-ops: M = 0, and n = 0 (the arrays may be NULL then and are not touched; the masses are still returned)
    assert lib.mlmc_density_sample_joint_batch(0, None, None, None, None, None, None, 0, 0, 0, None, 1, None, 0, 5, 0, None, None, None,
                                               None, hip.HOST) == 0
    out[:] = 7.25
    assert raw(n=0) == 0 and raw(n=0, out=None) == 0 and np.all(out == 7.25)
    mass = np.full(4, -1.0)
    assert raw(n=0, out=None, mass=mass) == 0
    assert np.array_equal(mass, _quantiles_c(hip, group, quad, np.zeros(0), [0] * 4)[1]) and np.all(mass > 0)


def test_joint_samples(hip, table):
    """joint_samples with corr == the C entry with correlation_factor(corr); device tensors hold the same bits"""
    import torch
    from mlmc_amd.tool import simple_distribution as sd
    group = table[1][:3]
    distrs = [p["dist"] for p in group]
    F, _ = sd.correlation_factor(jc.CORR3)
    want, want_u, want_z, _ = _ok(hip, group, F, 257, first=3, flags=1)
    x, u, z = sd.joint_samples(distrs, 257, SEED, corr=jc.CORR3, first=3, antithetic=True, return_uniforms=True, return_normals=True)
    assert _same(x, want) and _same(u, want_u) and _same(z, want_z)
    assert _same(sd.joint_samples(distrs, 257, SEED, factor=F, first=3, antithetic=True), want)
    xd, ud, zd = sd.joint_samples(distrs, 257, SEED, corr=jc.CORR3, first=3, antithetic=True, device=True, return_uniforms=True,
                                  return_normals=True)
    for d, w in ((xd, want), (ud, want_u), (zd, want_z)):
        assert isinstance(d, torch.Tensor) and d.is_cuda and d.dtype == torch.float64 and _same(d.cpu().numpy(), w)
    x2, z2 = sd.joint_samples(distrs, 64, SEED, factor=np.ones((3, 1)), streams=[4], return_normals=True)
    assert x2.shape == (3, 64) and z2.shape == (1, 64) and _same(z2, _ok(hip, group, np.ones((3, 1)), 64, streams=[4])[2])
    assert sd.joint_samples(distrs, 0, SEED, corr=jc.CORR3).shape == (3, 0)
    mixed = [distrs[0], table[0][1]["dist"], distrs[2]]
    with pytest.raises(ValueError, match="same quadrature"):
        sd.joint_samples(mixed, 4, SEED, corr=jc.CORR3)


def test_estimate_sample_joint(hip):
    import torch
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.tool import simple_distribution as sd
    dev, spec, M = _small_vector_storage()
    qe.device_cache_clear()
    q = make_root_quantity(dev, spec)['q']
    doms = Estimate.estimate_domains(q, dev)
    fns = [Legendre(7, tuple(doms[m])) for m in range(M)]
    est = Estimate(q, dev, fns[0])
    pdfs = est.construct_densities(tol=1e-8, orth_moments_tol=1e-4, moments_fns=fns)
    distrs = [d[0] for d in pdfs]
    n = 1000
    draws, ok, used = est.sample_joint(n, SEED, densities=pdfs)
    assert draws.shape == (M, n) and draws.dtype == np.float64 and ok.shape == (M,) and ok.dtype == bool and used.shape == (M, M)
    assert np.array_equal(ok, np.array([bool(d[2].success) for d in pdfs]))
    cov, _ = est.estimate_component_covariance()
    s = np.sqrt(np.diag(cov))
    corr = cov / s[:, None] / s[None, :]
    np.fill_diagonal(corr, 1.0)
    F, _ = sd.correlation_factor(corr)
    assert np.array_equal(used, F @ F.T) and np.allclose(np.diag(used), 1.0, atol=1e-15)
    assert _same(draws, sd.joint_samples(distrs, n, SEED, factor=F))
    for m in range(M):
        assert np.all((draws[m] >= doms[m][0]) & (draws[m] <= doms[m][1]))
    fresh, ok2, used2 = est.sample_joint(n, SEED, tol=1e-8, orth_moments_tol=1e-4, moments_fns=fns)
    assert _same(fresh, draws) and np.array_equal(ok2, ok) and np.array_equal(used2, used)
    on_dev, _, _ = est.sample_joint(n, SEED, densities=pdfs, device=True)
    assert isinstance(on_dev, torch.Tensor) and on_dev.is_cuda and on_dev.shape == (M, n) and _same(on_dev.cpu().numpy(), draws)
    cont, _, _ = est.sample_joint(100, SEED, densities=pdfs, first=900, antithetic=True)
    assert _same(cont, sd.joint_samples(distrs, 100, SEED, factor=F, first=900, antithetic=True))
    # corr = identity: the uniforms are those of sample_components up to the rounding of Phi(Phi^-1(u0)), which is at most
    # phi(z) dz + E_Phi with dz the error of normcdfinv
    eye, _, used_eye = est.sample_joint(n, SEED, corr=np.eye(M), densities=pdfs)
    assert np.array_equal(used_eye, np.eye(M))
    x, u = sd.joint_samples(distrs, n, SEED, corr=np.eye(M), return_uniforms=True)
    assert _same(x, eye)
    u0 = np.array([sc.uniforms(SEED, m, 0, n) for m in range(M)])
    zr = special.ndtri(u0)
    bound = np.exp(-0.5 * zr * zr) / np.sqrt(2 * np.pi) * jc.z_tolerance() * U * np.maximum(1.0, np.abs(zr)) * 1.01 \
        + jc.phi_tolerance() * U * u0 * 1.01
    assert np.all(np.abs(u - u0) <= bound)
    # a component without a positive variance estimate
    zero = cov.copy()
    zero[2, :] = zero[:, 2] = 0.0
    est.estimate_component_covariance = lambda: (zero, None)
    with pytest.raises(ValueError, match="component 2"):
        est.sample_joint(n, SEED, densities=pdfs)
    with pytest.raises(ValueError, match="n must be"):
        est.sample_joint(-1, SEED, corr=np.eye(M), densities=pdfs)
