"""GPU tests of the Student-t copula (mlmc_amd/csrc/copula_t.hip, the TSCALE instance of k_cop_uniforms in copula.hip) through
mlmc_student_t_cdf, mlmc_chi2_mixing_scale, mlmc_density_sample_joint_t_batch and simple_distribution.joint_samples(dof=...).

u = clamp(T_nu((F z) s)), s = chi2_mixing_scale(nu, p0) (include/mlmc_hip.h).  The two functions are compared with mpmath at the
arguments of tests/t_copula_cases.py, the mixing scales and the map with the elementwise entries bit for bit, the product with a
long-double dot of the device's own normals, the structure bit for bit, and the draws' concordance with the t orthant."""
import ctypes as C

import mpmath
import numpy as np
import pytest
from scipy import special

from tests import concordance_cases as cc
from tests import joint_sample_cases as jc
from tests import maxent_cases as mc
from tests import quantile_cases as qc
from tests import sample_cases as sc
from tests import t_copula_cases as tc
from tests.test_gpu_density_samples import CASES, SEED, _quantiles_c, _same
from tests.test_gpu_quantiles import _dist, _fn, _raw_args

pytestmark = pytest.mark.gpu
U = jc.U
ANTITHETIC, SOBOL = 1, 8


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    assert _lib.SAMPLE_ANTITHETIC == ANTITHETIC and _lib.SAMPLE_SOBOL == SOBOL
    return _lib


@pytest.fixture(scope="module")
def group6(hip):
    """the six cases of the sampling tests under the first rule of qc.RULES at the multipliers the device solver returns"""
    from mlmc_amd.tool import simple_distribution as sd
    quad = qc.RULES[0]
    group = []
    for name in CASES:
        case = mc.cases()[name]
        lam, _, _, info = sd._solve_on_device(_fn(case), case.mu, case.sigma, case.domain, case.lam0, 1e-8, 100, n_intervals=quad[0],
                                              gauss_degree=quad[1])
        assert info.success == 1, name
        group.append(dict(case=case, lam=lam, quad=quad, dist=_dist(case, lam, quad), tag=name))
    return group


def _last_error(hip):
    return hip.lib().mlmc_last_error().decode()


def _cycle(group, M):
    return [group[i % len(group)] for i in range(M)]


def _joint_t(hip, group, F, n, dof, seed=SEED, streams=None, mix_stream=None, first=0, flags=0, kind=None, want_s=True):
    """mlmc_density_sample_joint_t_batch on the problems of `group`; returns (rc, out [M, n], u [M, n], z [K, n], s [n])"""
    import torch
    kind = hip.HOST if kind is None else kind
    M = len(group)
    F = np.ascontiguousarray(F, dtype=np.float64)
    K = F.shape[1]
    handles, r1, lam, sig = _raw_args(hip, group)
    a = np.array([p["case"].domain[0] for p in group], dtype=np.float64)
    b = np.array([p["case"].domain[1] for p in group], dtype=np.float64)
    st = None if streams is None else np.ascontiguousarray(streams, dtype=np.uint32)
    mix_stream = K if mix_stream is None else mix_stream
    cols = max(int(n), 0)

    def array(shape, want=True):
        if not want:
            return None
        if kind == hip.DEVICE:
            return torch.full(shape, 7.25, dtype=torch.float64, device="cuda")
        return np.full(shape, 7.25)
    out, u, z, s = array((M, cols)), array((M, cols)), array((K, cols)), array((cols,), want_s)
    if kind == hip.DEVICE:
        torch.cuda.synchronize()
    quad = group[0]["quad"]
    rc = hip.lib().mlmc_density_sample_joint_t_batch(M, C.cast(handles, C.c_void_p), hip.ptr(r1), hip.ptr(lam), hip.ptr(sig), hip.ptr(a),
                                                     hip.ptr(b), quad[0], quad[1], K, hip.ptr(F), float(dof), seed, hip.ptr(st),
                                                     mix_stream, first, n, flags, hip.ptr(out), hip.ptr(u), hip.ptr(z), hip.ptr(s), None,
                                                     kind)
    if kind == hip.DEVICE:
        out, u, z, s = (None if v is None else v.cpu().numpy() for v in (out, u, z, s))
    return rc, out, u, z, s


def _ok(hip, *args, **kw):
    rc, out, u, z, s = _joint_t(hip, *args, **kw)
    hip.check(rc)
    return out, u, z, s


def _entry(hip, name, dof, x, kind=None):
    """one of the elementwise entries on a 1-D array -> (rc, result)"""
    import torch
    x = np.ascontiguousarray(x, dtype=np.float64)
    fn = getattr(hip.lib(), name)
    if kind == hip.DEVICE:
        xd = torch.from_numpy(x).cuda()
        out = torch.full_like(xd, 7.25)
        torch.cuda.synchronize()
        rc = fn(float(dof), x.size, hip.ptr(xd), hip.ptr(out), hip.DEVICE)
        return rc, out.cpu().numpy()
    out = np.full(x.shape, 7.25)
    return fn(float(dof), x.size, hip.ptr(x), hip.ptr(out), hip.HOST), out


def _t_cdf(hip, dof, y, kind=None):
    rc, out = _entry(hip, "mlmc_student_t_cdf", dof, y, kind)
    hip.check(rc)
    return out


def _scale(hip, dof, p, kind=None):
    rc, out = _entry(hip, "mlmc_chi2_mixing_scale", dof, p, kind)
    hip.check(rc)
    return out


# ---- the elementwise entries -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dof", tc.DOFS)
def test_elementwise_entries_against_mpmath(hip, dof):
    y = tc.t_arguments(dof)
    u = _t_cdf(hip, dof, y)
    units = tc.t_units(u, tc.mp_t_cdf(dof, y))
    k = int(np.argmax(units))
    p = tc.p_arguments()
    s = _scale(hip, dof, p)
    s_units = tc.s_units(dof, p, s)
    i = int(np.argmax(s_units))
    print(f"\nnu {dof:g}: student_t_cdf worst {units[k]:.4g} units at y = {y[k]!r} (recorded {tc.T_UNITS_OBSERVED}, tolerance "
          f"{jc.tolerance(tc.T_UNITS_OBSERVED):g}); chi2_mixing_scale worst {s_units[i]:.4g} units at p = {p[i]!r} (recorded "
          f"{tc.S_UNITS_OBSERVED}, tolerance {jc.tolerance(tc.S_UNITS_OBSERVED):g})")
    assert units[k] <= jc.tolerance(tc.T_UNITS_OBSERVED)
    assert s_units[i] <= jc.tolerance(tc.S_UNITS_OBSERVED)
    assert np.all(np.isfinite(s) & (s > 0.0))
    # device memory gives the same bits; cdf(y) == 1 - cdf(-y) bit for bit for y > 0
    assert _same(_t_cdf(hip, dof, y, hip.DEVICE), u) and _same(_scale(hip, dof, p, hip.DEVICE), s)
    pos = y > 0.0
    assert _same(u[pos], 1.0 - _t_cdf(hip, dof, -y[pos]))
    special_u = _t_cdf(hip, dof, [-np.inf, np.inf, np.nan, 0.0, -0.0])
    assert special_u[0] == 0.0 and special_u[1] == 1.0 and np.isnan(special_u[2]) and special_u[3] == 0.5 and special_u[4] == 0.5
    assert np.all(np.isnan(_scale(hip, dof, [0.0, 1.0, -0.25, 1.5, np.nan, np.inf])))


def test_elementwise_errors_and_no_ops(hip):
    x = np.array([0.25, 0.5])
    for name in ("mlmc_student_t_cdf", "mlmc_chi2_mixing_scale"):
        fn = getattr(hip.lib(), name)
        out = np.full(2, 7.25)
        for bad in (0.999, 64.001, np.nan, np.inf, -3.0):
            assert fn(bad, 2, hip.ptr(x), hip.ptr(out), hip.HOST) != 0 and "dof must lie in [1, 64]" in _last_error(hip)
        assert fn(3.0, -1, hip.ptr(x), hip.ptr(out), hip.HOST) != 0 and "n < 0" in _last_error(hip)
        assert fn(3.0, 2, None, hip.ptr(out), hip.HOST) != 0 and "null argument" in _last_error(hip)
        assert fn(3.0, 2, hip.ptr(x), None, hip.HOST) != 0 and "null argument" in _last_error(hip)
        assert fn(3.0, 2, hip.ptr(x), hip.ptr(out), 7) != 0 and "bad mem_kind" in _last_error(hip)
        assert fn(3.0, 0, hip.ptr(x), hip.ptr(out), hip.HOST) == 0 and np.all(out == 7.25)
        assert fn(1.0, 2, hip.ptr(x), hip.ptr(out), hip.HOST) == 0 and fn(64.0, 2, hip.ptr(x), hip.ptr(out), hip.HOST) == 0


def test_python_elementwise_entries(hip):
    import torch
    from mlmc_amd.tool import simple_distribution as sd
    y = np.array([[-3.0, 0.0], [0.5, 40.0]])
    u = sd.student_t_cdf(y, 4.5)
    assert u.shape == (2, 2) and _same(u.ravel(), _t_cdf(hip, 4.5, y.ravel()))
    ud = sd.student_t_cdf(torch.from_numpy(y).cuda(), 4.5, device=True)
    assert ud.is_cuda and _same(ud.cpu().numpy(), u)
    p = np.array([0.01, 0.5, 0.99])
    assert _same(sd.chi2_mixing_scale(p, 3), _scale(hip, 3, p))
    assert abs(float(sd.student_t_cdf(-1.0, 1.0)) - 0.25) < 1e-15 and isinstance(sd.chi2_mixing_scale(0.5, 2), float)


# ---- mixing, map, inversion --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, ANTITHETIC, SOBOL])
def test_mixing_scales(hip, group6, flags):
    """s_out == mlmc_chi2_mixing_scale at the host restatement of the mixing uniform, bit for bit"""
    group, F = _cycle(group6, 3), jc.random_factor(np.random.default_rng(3), 3, 2)
    for first in (0, 50):
        for dof, mix_stream in ((3.0, 2), (30.0, 977)):
            _, _, z, s = _ok(hip, group, F, 130, dof, mix_stream=mix_stream, first=first, flags=flags)
            p0 = tc.mixing_uniforms(SEED, mix_stream, first, 130, antithetic=flags == ANTITHETIC, qmc=flags == SOBOL)
            assert _same(s, _scale(hip, dof, p0)), (flags, first, dof)
            if flags == ANTITHETIC:
                assert _same(s[0::2], s[1::2]) and _same(z[:, 0::2], -z[:, 1::2])
            # the latent normals are those of the Gaussian entry
            if flags == SOBOL:
                from tests import sobol_cases
                want = sobol_cases.normals(SEED, [0, 1], first, 130)
            else:
                want = jc.normals(SEED, [0, 1], first, 130, antithetic=flags == ANTITHETIC)
            assert np.max(np.abs(z - want)) <= jc.z_tolerance() * U * np.max(np.maximum(1.0, np.abs(want)))


@pytest.mark.parametrize("dof", [1.0, 3.0, 30.0])
def test_map_and_inversion(hip, group6, dof):
    """F = I: the chain is exact, so u_out == clamp(mlmc_student_t_cdf(z_out * s_out)) with the product formed on the host, and
    out == the quantile entry at u_out, bit for bit; host and device arrays"""
    group = _cycle(group6, 5)
    for kind in (hip.HOST, hip.DEVICE):
        out, u, z, s = _ok(hip, group, np.eye(5), 400, dof, first=3, kind=kind)
        assert _same(u, tc.clamp(_t_cdf(hip, dof, (z * s[None, :]).ravel())).reshape(5, 400)), kind
        assert np.all((u >= jc.U_LO) & (u <= jc.U_HI))
        want, _ = _quantiles_c(hip, group, group[0]["quad"], u.ravel(), [400] * 5)
        assert _same(out.ravel(), want) and np.all(np.isfinite(out))


def _mp_t_cdf_ld(dof, y):
    """T_nu at long-double numbers, a list of mpf"""
    out = []
    with mpmath.workdps(tc.MP_DIGITS):
        nu, half = mpmath.mpf(float(dof)), mpmath.mpf(1) / 2
        for v in np.ravel(y):
            t = jc._mpf(v)
            if t * t < nu:
                low = (1 - mpmath.betainc(half, nu / 2, 0, t * t / (nu + t * t), regularized=True)) / 2
            else:
                low = mpmath.betainc(nu / 2, half, 0, nu / (nu + t * t), regularized=True) / 2
            out.append(low if t <= 0 else 1 - low)
    return out


@pytest.mark.parametrize("M,K,n,first,dof", [(1, 1, 1, 0, 1.0), (17, 5, 130, 50, 3.0), (65, 33, 65, 0, 30.0), (17, 33, 63, 50, 1.0),
                                             (65, 1, 63, 0, 3.0), (1, 5, 130, 0, 30.0)])
def test_product_and_epilogue(hip, group6, M, K, n, first, dof):
    """random row-normalised F: u_out against T_nu of (the long-double dot of F with the device's own z_out) x s_out, within the
    first-order bound of test_gemm_and_epilogue with the t density f_nu(y) in the place of the normal one,
        f_nu(y) [ (K + 2) 2^-53 s sum_k |F_mk z_k|  +  2^-53 |y| ]  +  E_T 2^-53 max(T, 2^-53):
    the chain's error scaled by s, the one rounded multiplication by s, and the error of the t CDF"""
    F = jc.random_factor(np.random.default_rng(100 * M + K), M, K)
    _, u, z, s = _ok(hip, _cycle(group6, M), F, n, dof, first=first)
    y = jc.ld_dot(F, z) * s.astype(jc.LD)[None, :]
    ref_mp = _mp_t_cdf_ld(dof, y)
    ref = np.array([float(v) for v in ref_mp]).reshape(M, n)
    err = jc.phi_abs_errors(u, ref_mp).reshape(M, n)
    yd = y.astype(np.float64)
    dens = np.exp(special.gammaln(0.5 * (dof + 1.0)) - special.gammaln(0.5 * dof)) / np.sqrt(dof * np.pi) \
        * (1.0 + yd * yd / dof) ** (-0.5 * (dof + 1.0))
    bound = dens * ((K + 2) * U * s[None, :] * (np.abs(F) @ np.abs(z)) + U * np.abs(yd)) \
        + jc.tolerance(tc.T_UNITS_OBSERVED) * U * np.maximum(ref, U)
    k = int(np.argmax(err / bound))
    print(f"\nM {M} K {K} n {n} nu {dof:g}: worst error / bound {(err / bound).ravel()[k]:.3g}")
    assert np.all(err <= bound)


# ---- structure ---------------------------------------------------------------------------------------------------------------

def test_structure(hip, group6, monkeypatch):
    rng = np.random.default_rng(7)
    group = _cycle(group6, 65)
    F = jc.random_factor(rng, 65, 33)
    dof = 3.0
    whole = _ok(hip, group, F, 150, dof)
    # first = 50, n = 100 gives columns [50, 150) of first = 0, n = 150
    part = _ok(hip, group, F, 100, dof, first=50)
    assert all(_same(a[..., 50:], b) for a, b in zip(whole, part))
    # blocks of 64 draws against one block; device against host arrays; without s_out
    monkeypatch.setenv("MLMC_JOINT_BLOCK_DRAWS", "64")
    assert all(_same(a, b) for a, b in zip(whole, _ok(hip, group, F, 150, dof)))
    assert all(_same(a, b) for a, b in zip(whole, _ok(hip, group, F, 150, dof, kind=hip.DEVICE)))
    monkeypatch.delenv("MLMC_JOINT_BLOCK_DRAWS")
    assert all(_same(a, b) for a, b in zip(whole, _ok(hip, group, F, 150, dof, kind=hip.DEVICE)))
    assert all(_same(a, b) for a, b in zip(whole[:3], _ok(hip, group, F, 150, dof, want_s=False)[:3]))
    # a row alone against the row inside M = 65 (mix_stream named: its default K is the same)
    for m in (0, 17, 64):
        alone = _ok(hip, [group[m]], F[m:m + 1], 150, dof, mix_stream=33)
        assert _same(alone[0][0], whole[0][m]) and _same(alone[1][0], whole[1][m]) and _same(alone[3], whole[3])
    # another nu, another mixing stream: other draws
    assert not _same(_ok(hip, group[:1], F[:1], 150, 4.0, mix_stream=33)[1], whole[1][:1])
    assert not _same(_ok(hip, group[:1], F[:1], 150, dof, mix_stream=34)[3], whole[3])


def test_antithetic_pairs(hip, group6):
    group, F = _cycle(group6, 17), jc.random_factor(np.random.default_rng(8), 17, 5)
    _, u, z, s = _ok(hip, group, F, 256, 3.0, flags=ANTITHETIC)
    assert _same(s[0::2], s[1::2]) and _same(z[:, 0::2], -z[:, 1::2])
    inside = (u[:, 0::2] > jc.U_LO) & (u[:, 0::2] < jc.U_HI) & (u[:, 1::2] > jc.U_LO) & (u[:, 1::2] < jc.U_HI)
    # y negates exactly, cdf(y) == 1 - cdf(-y) bit for bit for y > 0: whichever of the pair has y > 0 is 1 - the other
    upper = np.maximum(u[:, 0::2], u[:, 1::2])
    lower = np.minimum(u[:, 0::2], u[:, 1::2])
    assert inside.sum() > 2000 and _same(upper[inside], 1.0 - lower[inside])


def test_the_gaussian_entry_is_untouched(hip, group6):
    from tests.test_gpu_joint_samples import _ok as gauss_ok
    group, F = _cycle(group6, 17), jc.random_factor(np.random.default_rng(9), 17, 5)
    before = gauss_ok(hip, group, F, 257, first=3)
    _ok(hip, group, F, 257, 3.0, first=3)
    after = gauss_ok(hip, group, F, 257, first=3)
    assert all(_same(a, b) for a, b in zip(before[:3], after[:3]))
    from mlmc_amd.tool import simple_distribution as sd
    distrs = [p["dist"] for p in group]
    plain = sd.joint_samples(distrs, 257, SEED, factor=F, first=3, return_uniforms=True)
    assert _same(plain[0], before[0]) and _same(plain[1], before[1])
    assert all(_same(a, b) for a, b in zip(plain, sd.joint_samples(distrs, 257, SEED, factor=F, first=3, return_uniforms=True, dof=np.inf)))


def test_errors_and_no_ops(hip, group6):
    group, F = _cycle(group6, 3), jc.random_factor(np.random.default_rng(10), 3, 2)
    for bad in (0.5, 64.5, np.nan):
        rc = _joint_t(hip, group, F, 8, bad)[0]
        assert rc != 0 and "dof must lie in [1, 64]" in _last_error(hip)
    rc = _joint_t(hip, group, F, 8, 3.0, mix_stream=1)[0]
    assert rc != 0 and "mix_stream equals the stream of latent normal 1" in _last_error(hip)
    rc = _joint_t(hip, group, F, 8, 3.0, streams=[5, 9], mix_stream=9)[0]
    assert rc != 0 and "mix_stream equals the stream of latent normal 1" in _last_error(hip)
    rc = _joint_t(hip, group, F, 8, 3.0, mix_stream=1024, flags=SOBOL)[0]
    assert rc != 0 and "mixing variable" in _last_error(hip)
    rc = _joint_t(hip, group, F, 8, 3.0, flags=ANTITHETIC | SOBOL)[0]
    assert rc != 0 and "exclude each other" in _last_error(hip)
    rc, out, u, z, s = _joint_t(hip, group, F, 0, 3.0)
    assert rc == 0
    rc = _joint_t(hip, group, F, -1, 3.0)[0]
    assert rc != 0 and "n < 0" in _last_error(hip)


def test_kernel_time_counts_one_launch_per_block(hip, group6, monkeypatch):
    group, F = _cycle(group6, 3), jc.random_factor(np.random.default_rng(11), 3, 2)
    ms, launches = C.c_double(-1.0), C.c_int64(-1)
    hip.check(hip.lib().mlmc_density_quantiles_kernel_time(C.byref(ms), C.byref(launches)))      # reads and resets
    _ok(hip, group, F, 150, 3.0)
    hip.check(hip.lib().mlmc_density_quantiles_kernel_time(C.byref(ms), C.byref(launches)))
    assert launches.value == 1 and ms.value > 0.0
    monkeypatch.setenv("MLMC_JOINT_BLOCK_DRAWS", "64")
    _ok(hip, group, F, 150, 3.0)
    hip.check(hip.lib().mlmc_density_quantiles_kernel_time(C.byref(ms), C.byref(launches)))
    assert launches.value == 3 and ms.value > 0.0


# ---- python entry and the statistics of the draws ----------------------------------------------------------------------------

def test_joint_samples_entry(hip, group6):
    from mlmc_amd.tool import simple_distribution as sd
    group, F = _cycle(group6, 3), jc.random_factor(np.random.default_rng(12), 3, 3)
    distrs = [p["dist"] for p in group]
    want = _ok(hip, group, F, 100, 4.5, first=6)
    got = sd.joint_samples(distrs, 100, SEED, factor=F, first=6, dof=4.5, return_uniforms=True, return_normals=True, return_mixing=True)
    assert len(got) == 4 and all(_same(a, b) for a, b in zip(got, want))
    x = sd.joint_samples(distrs, 100, SEED, factor=F, first=6, dof=4.5, device=True)
    assert x.is_cuda and _same(x.cpu().numpy(), want[0])
    x, s = sd.joint_samples(distrs, 100, SEED, factor=F, first=6, dof=4.5, streams=[0, 1, 2], mix_stream=3, return_mixing=True)
    assert _same(x, want[0]) and _same(s, want[3])
    agg = sd.joint_aggregates(distrs, 100, SEED, weights=np.ones(3), factor=F, first=6, dof=4.5, block=32)
    assert _same(agg.rows, sd.scenario_aggregates(want[0], weights=np.ones(3)).rows)


def _uniform_distributions():
    from tests import score_cases as sk
    return [sk.closed_distribution(0.0, (0.0, 1.0)) for _ in range(3)]


def _device_z(hip, u_device, n):
    from mlmc_amd.tool import simple_distribution as sd
    lower, upper = cc.upper_events(tc.STAT_PROBS, 3)
    counts = sd.concordance_counts(u_device, None, lower, upper)
    assert int(counts.kept[0]) == n
    return tc.concordance_z(counts.pair, counts.kept[0])


def _dkw(u):
    """the Kolmogorov distance of every row from the uniform law"""
    n = u.shape[1]
    srt = np.sort(u, axis=1)
    grid = np.arange(1, n + 1) / n
    return np.maximum(np.max(np.abs(srt - grid), axis=1), np.max(np.abs(srt - (grid - 1.0 / n)), axis=1))


def test_statistics_of_the_draws(hip):
    """the concordance of the device's own uniforms, counted on the device: the t orthant fits, the normal one does not"""
    from mlmc_amd.tool import simple_distribution as sd
    distrs = _uniform_distributions()
    _, u = sd.joint_samples(distrs, tc.STAT_N, tc.STAT_SEED, corr=cc.CORR, dof=tc.STAT_DOF, device=True, return_uniforms=True)
    res = _device_z(hip, u, tc.STAT_N)
    print("\nPhilox: |z| under the t model", np.round(np.abs(res["z_t"]).max(axis=1), 2), "z under the Gaussian model at 0.9",
          np.round(res["z_gauss"][1], 2))
    assert np.max(np.abs(res["z_t"])) < tc.STAT_Z_BOUND and np.min(res["z_gauss"][1]) > tc.STAT_Z_GAUSS
    assert res["fit"].dof == tc.STAT_DOF
    # DKW at confidence 1 - 1e-9 for n draws: sqrt(log(2 / 1e-9) / (2 n))
    d = _dkw(u.cpu().numpy())
    bound = np.sqrt(np.log(2.0 / 1e-9) / (2.0 * tc.STAT_N))
    print("Kolmogorov distances of the rows", np.round(d, 5), "bound", round(float(bound), 5))
    assert np.all(d <= bound + 1e-9)


def test_statistics_of_the_sobol_draws(hip):
    """8 scrambles of 2^15 points, their counts added up on the device: 2^18 draws held to the bounds of 2^18 independent ones (a
    scrambled net is no worse than that for an indicator)"""
    from mlmc_amd.tool import simple_distribution as sd
    distrs = _uniform_distributions()
    lower, upper = cc.upper_events(tc.STAT_PROBS, 3)
    counts = None
    bound = np.sqrt(np.log(2.0 / 1e-9) / (2.0 * tc.STAT_SOBOL_N))
    for seed in tc.STAT_SOBOL_SEEDS:
        _, u = sd.joint_samples(distrs, tc.STAT_SOBOL_N, seed, corr=cc.CORR, dof=tc.STAT_DOF, device=True, return_uniforms=True, qmc=True)
        counts = sd.concordance_counts(u, None, lower, upper, device=True, out=counts)
        assert np.all(_dkw(u.cpu().numpy()) <= bound + 1e-9)
    n = len(tc.STAT_SOBOL_SEEDS) * tc.STAT_SOBOL_N
    assert int(counts.kept[0]) == n
    res = tc.concordance_z(counts.pair.cpu().numpy(), n)
    print("\nSobol': |z| under the t model", np.round(np.abs(res["z_t"]).max(axis=1), 2), "z under the Gaussian model at 0.9",
          np.round(res["z_gauss"][1], 2))
    assert np.max(np.abs(res["z_t"])) < tc.STAT_Z_BOUND and np.min(res["z_gauss"][1]) > tc.STAT_Z_GAUSS
    assert res["fit"].dof == tc.STAT_DOF
