"""GPU tests of the conditional joint draws under the Gaussian copula (the SHIFT instance of k_cop_uniforms in
mlmc_amd/csrc/copula.hip, the SETS instances of k_q_sample and q_copula with sets in density.hip) through
mlmc_density_sample_conditional_batch, simple_distribution.conditional_samples / conditional_quantiles / conditional_cdfs and
Estimate.sample_conditional / estimate_conditional_quantiles.

x[b][m][j] = Q_m(u), u = clamp(Phi(shift[b][m] (+) (F z)[m][j])) (include/mlmc_hip.h).  With a zero shift the entry is compared bit for
bit with the joint entry, the shifted epilogue with mpmath at the device's own normals, the structure and the inversion bit for
bit, the conditional law with the restatement of tests/conditional_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy import special

from tests import conditional_cases as cc
from tests import joint_sample_cases as jc
from tests import quantile_cases as qc
from tests import sample_cases as sc
from tests.test_gpu_density_samples import FAR, SEED, _quantiles_c, _same, _small_vector_storage
from tests.test_gpu_joint_samples import _cycle, _ok, hip, table  # noqa: F401  (fixtures)
from tests.test_gpu_quantiles import _fn, _raw_args

pytestmark = pytest.mark.gpu
NAME = "mlmc_density_sample_conditional_batch"
U = jc.U
SENTINEL = 7.25


def _cond(hip, group, F, n, B=1, shift=None, rows=None, ld_rows=None, seed=SEED, streams=None, first=0, flags=0, kind=None,
          want_u=True, want_z=True, want_mass=False):
    """mlmc_density_sample_conditional_batch on the problems of `group`; returns (rc, out [B, ld_rows, n], u [B, ld_rows, n],
    z [K, n], mass); the arrays are filled with SENTINEL before the call"""
    import torch
    kind = hip.HOST if kind is None else kind
    M = len(group)
    F = np.ascontiguousarray(F, dtype=np.float64)
    K = F.shape[1]
    handles, r1, lam, sig = _raw_args(hip, group)
    a = np.array([p["case"].domain[0] for p in group], dtype=np.float64)
    b = np.array([p["case"].domain[1] for p in group], dtype=np.float64)
    st = None if streams is None else np.ascontiguousarray(streams, dtype=np.uint32)
    sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
    rw = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
    ld = M if ld_rows is None else ld_rows
    cols, sets, height = max(int(n), 0), max(int(B), 1), max(ld, M)

    def array(shape, want):
        if not want:
            return None
        if kind == hip.DEVICE:
            return torch.full(shape, SENTINEL, dtype=torch.float64, device="cuda")
        return np.full(shape, SENTINEL)
    out, u, z = array((sets, height, cols), True), array((sets, height, cols), want_u), array((K, cols), want_z)
    if kind == hip.DEVICE:
        torch.cuda.synchronize()
    mass = np.full(M, -1.0) if want_mass else None
    quad = group[0]["quad"]
    rc = hip.lib().mlmc_density_sample_conditional_batch(
        M, C.cast(handles, C.c_void_p), hip.ptr(r1), hip.ptr(lam), hip.ptr(sig), hip.ptr(a), hip.ptr(b), quad[0], quad[1], K, hip.ptr(F),
        seed, hip.ptr(st), first, n, flags, B, hip.ptr(sh), hip.ptr(rw), ld, hip.ptr(out), hip.ptr(u), hip.ptr(z), hip.ptr(mass), kind)
    if kind == hip.DEVICE:
        out, u, z = (None if v is None else v.cpu().numpy() for v in (out, u, z))
    return rc, out, u, z, mass


def _cok(hip, *args, **kw):
    rc, out, u, z, mass = _cond(hip, *args, **kw)
    hip.check(rc)
    return out, u, z, mass


def _scaled_factor(rng, M, K):
    """random rows scaled by factors in [0, 1]: one row (the last of the first row tile's ragged part) exactly zero, one of norm 1"""
    F = jc.random_factor(rng, M, K) * rng.uniform(0.0, 1.0, M)[:, None]
    F[M // 2] = 0.0
    if M > 1:
        F[0] = jc.random_factor(rng, 1, K)[0]
    return np.ascontiguousarray(F)


@pytest.mark.parametrize("M,K,n,first", [(1, 1, 17, 0), (17, 5, 257, 3), (65, 65, 65, 0)])
def test_reduction_to_the_joint_entry(hip, table, M, K, n, first):
    """B = 1 with a NULL shift and with explicit zeros, unit-norm F: out, u_out and z_out are the joint entry's bits"""
    group = _cycle(table[1], M)
    F = jc.random_factor(np.random.default_rng(100 * M + K), M, K)
    want = _ok(hip, group, F, n, first=first)[:3]
    for shift in (None, np.zeros((1, M))):
        for kind in (hip.HOST, hip.DEVICE):
            out, u, z, _ = _cok(hip, group, F, n, first=first, shift=shift, kind=kind)
            assert _same(out[0], want[0]) and _same(u[0], want[1]) and _same(z, want[2]), (shift is None, kind)
    out, u, z, _ = _cok(hip, group, F, n, first=first, flags=1)
    want = _ok(hip, group, F, n, first=first, flags=1)[:3]
    assert _same(out[0], want[0]) and _same(u[0], want[1]) and _same(z, want[2])


@pytest.mark.parametrize("M,K,n,B", [(1, 1, 17, 1), (3, 3, 1000, 2), (17, 5, 257, 3), (65, 65, 65, 2), (16, 17, 64, 5)])
def test_shifted_epilogue(hip, table, M, K, n, B):
    """rows of F scaled into [0, 1] (one exactly zero), shifts in [-3, 3]: u_out against Phi (mpmath) of shift + the long-double
    dot of F with the device's own z_out, within the bound of test_gemm_and_epilogue plus one rounding of the addition,
    phi(y) ((K + 2) 2^-53 sum_k |F_mk z_k| + 2^-53 |y|) + E_Phi"""
    rng = np.random.default_rng(1000 * M + 10 * K + B)
    F = _scaled_factor(rng, M, K) if M > 1 else np.array([[0.6]])
    shift = rng.uniform(-3.0, 3.0, (B, M))
    _, u, z, _ = _cok(hip, _cycle(table[1], M), F, n, B=B, shift=shift)
    dot = jc.ld_dot(F, z)
    absdot = np.abs(F) @ np.abs(z)
    worst = 0.0
    for b in range(B):
        y = shift[b].astype(jc.LD)[:, None] + dot
        phi = jc.mp_ncdf(y)
        ref = np.array([float(v) for v in phi]).reshape(M, n)
        err = jc.phi_abs_errors(u[b], phi).reshape(M, n)
        yd = y.astype(np.float64)
        dens = np.exp(-0.5 * yd * yd) / np.sqrt(2 * np.pi)
        bound = dens * ((K + 2) * U * absdot + U * np.abs(yd)) + jc.phi_tolerance() * U * np.maximum(ref, U)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (b, float(np.max(err / bound)))
    print(f"\nM {M} K {K} n {n} B {B}: worst error / bound {worst:.3g}")


def test_exact_structure(hip, table):
    """a zero row, equal shifts, a set alone against the set among five, a permutation of the sets, shifts of +-40, rows / ld_rows"""
    rng = np.random.default_rng(21)
    M, K, n, B = 17, 5, 257, 5
    group = _cycle(table[0], M)
    quad = group[0]["quad"]
    F = _scaled_factor(rng, M, K)
    shift = rng.uniform(-3.0, 3.0, (B, M))
    shift[3] = shift[1]                                                     # two sets with equal shifts
    out, u, z, _ = _cok(hip, group, F, n, B=B, shift=shift)
    zero = M // 2
    assert np.all(F[zero] == 0.0)
    for b in range(B):
        assert np.all(u[b, zero] == u[b, zero, 0]) and np.all(out[b, zero] == out[b, zero, 0])
        ref = float(jc.mp_ncdf([shift[b, zero]])[0])
        assert abs(u[b, zero, 0] - ref) <= jc.phi_tolerance() * U * ref
        want, _ = _quantiles_c(hip, [group[zero]], quad, u[b, zero, :1], [1])
        assert out[b, zero, 0] == want[0]
    assert _same(out[3], out[1]) and _same(u[3], u[1]) and not _same(u[0], u[1])
    for b in (0, 2, 4):
        alone = _cok(hip, group, F, n, B=1, shift=shift[b:b + 1])
        assert _same(alone[0][0], out[b]) and _same(alone[1][0], u[b]) and _same(alone[2], z), b
    perm = np.array([4, 0, 3, 1, 2])
    for kind in (hip.HOST, hip.DEVICE):
        got = _cok(hip, group, F, n, B=B, shift=shift[perm], kind=kind)
        assert _same(got[0], out[perm]) and _same(got[1], u[perm]) and _same(got[2], z), kind
    # |shift| = 40: the clamps exactly, x finite and inside the domain
    far = np.stack([np.full(M, 40.0), np.full(M, -40.0)])
    o40, u40, _, _ = _cok(hip, group, F, 65, B=2, shift=far)
    assert np.all(u40[0] == 1.0 - U) and np.all(u40[1] == U) and np.all(np.isfinite(o40))
    for m, p in enumerate(group):
        a, b = p["case"].domain
        assert np.all((o40[:, m] >= a) & (o40[:, m] <= b)) and np.all(o40[0, m] > o40[1, m])
    # rows = [1, 3, 4] of 6: the named rows are the identity layout's rows, the others keep the sentinel
    sub, Fs, shs = group[:3], F[:3], shift[:, :3]
    ident = _cok(hip, sub, Fs, n, B=B, shift=shs)
    for kind in (hip.HOST, hip.DEVICE):
        for want_u in (True, False):
            got = _cok(hip, sub, Fs, n, B=B, shift=shs, rows=[1, 3, 4], ld_rows=6, kind=kind, want_u=want_u)
            arrays = ((got[0], ident[0]), (got[1], ident[1])) if want_u else ((got[0], ident[0]),)
            for g, w in arrays:
                assert g.shape == (B, 6, n) and _same(g[:, [1, 3, 4]], w) and np.all(g[:, [0, 2, 5]] == SENTINEL), (kind, want_u)
            assert _same(got[2], ident[2])
    # the identity written out, and a wider leading dimension
    got = _cok(hip, sub, Fs, n, B=B, shift=shs, rows=[0, 1, 2], ld_rows=4)
    assert _same(got[0][:, :3], ident[0]) and np.all(got[0][:, 3] == SENTINEL) and _same(got[1][:, :3], ident[1])


def test_inversion(hip, table):
    """out == mlmc_density_quantiles_batch(u_out) bit for bit, row (b, m) against problem m, and the masses are equal; both rules,
    host and device arrays, with and without u_out / z_out"""
    rng = np.random.default_rng(9)
    for group6 in table:
        quad = group6[0]["quad"]
        for M, K, n, first, B in ((17, 5, 255, 3, 3), (3, 3, 1000, 0, 2), (65, 4, 63, FAR, 2), (1, 1, 1, 0, 1)):
            group = _cycle(group6, M)
            F = _scaled_factor(rng, M, K) if M > 1 else np.array([[0.5]])
            shift = rng.uniform(-3.0, 3.0, (B, M))
            out, u, z, mass = _cok(hip, group, F, n, B=B, shift=shift, first=first, want_mass=True)
            for b in range(B):
                want, want_mass = _quantiles_c(hip, group, quad, u[b].ravel(), [n] * M)
                assert _same(out[b].ravel(), want) and np.array_equal(mass, want_mass), (quad, M, K, n, b)
            assert np.all(np.isfinite(out)) and np.all(mass > 0)
            for kind in (hip.HOST, hip.DEVICE):
                for want_u, want_z in ((True, True), (False, False), (True, False), (False, True)):
                    o, uu, zz, _ = _cok(hip, group, F, n, B=B, shift=shift, first=first, kind=kind, want_u=want_u, want_z=want_z)
                    assert _same(o, out) and (uu is None or _same(uu, u)) and (zz is None or _same(zz, z)), (quad, M, K, n, kind)


def test_independence(hip, table):
    """first = 50, n = 100 == [50, 150) of n = 150; a subset of the problems; the block length of the draws with B = 3; the launch
    count per block"""
    rng = np.random.default_rng(11)
    M, K, B = 20, 5, 3
    group = _cycle(table[1], M)
    F = _scaled_factor(rng, M, K)
    shift = rng.uniform(-3.0, 3.0, (B, M))
    whole = _cok(hip, group, F, 150, B=B, shift=shift)[:3]
    part = _cok(hip, group, F, 100, B=B, shift=shift, first=50)[:3]
    assert _same(part[0], whole[0][:, :, 50:]) and _same(part[1], whole[1][:, :, 50:]) and _same(part[2], whole[2][:, 50:])
    sub = _cok(hip, group[3:19], F[3:19], 150, B=B, shift=shift[:, 3:19])
    assert _same(sub[0], whole[0][:, 3:19]) and _same(sub[1], whole[1][:, 3:19]) and _same(sub[2], whole[2])
    alone = _cok(hip, [group[7]], F[7:8], 150, B=B, shift=shift[:, 7:8])
    assert _same(alone[0][:, 0], whole[0][:, 7]) and _same(alone[1][:, 0], whole[1][:, 7])
    # block seams: 257 draws in blocks of 96 (96 + 96 + 65)
    group, F, shift = group[:17], _scaled_factor(rng, 17, 17), shift[:, :17]
    want = _cok(hip, group, F, 257, B=B, shift=shift, first=3)[:3]
    assert "MLMC_JOINT_BLOCK_DRAWS" not in os.environ
    os.environ["MLMC_JOINT_BLOCK_DRAWS"] = "96"
    try:
        for kind in (hip.HOST, hip.DEVICE):
            got = _cok(hip, group, F, 257, B=B, shift=shift, first=3, kind=kind)[:3]
            assert all(_same(g, w) for g, w in zip(got, want)), kind
            assert _same(_cok(hip, group, F, 257, B=B, shift=shift, first=3, kind=kind, want_u=False, want_z=False)[0], want[0]), kind
        ms, launches = C.c_double(), C.c_int64()
        hip.check(hip.lib().mlmc_density_quantiles_kernel_time(C.byref(ms), C.byref(launches)))
        _cok(hip, group, F, 257, B=B, shift=shift)
        hip.check(hip.lib().mlmc_density_quantiles_kernel_time(C.byref(ms), C.byref(launches)))
        assert launches.value == 3 and ms.value > 0              # one per block, whatever B
    finally:
        del os.environ["MLMC_JOINT_BLOCK_DRAWS"]
    _cok(hip, group, F, 257, B=B, shift=shift)
    hip.check(hip.lib().mlmc_density_quantiles_kernel_time(C.byref(ms), C.byref(launches)))
    assert launches.value == 1


@pytest.mark.parametrize("first", [0, FAR])
def test_statistics_of_the_device_draws(hip, table, first):
    """jc.CORR3 and three marginals at n = 16384, the observed sets and scores of cc.STAT_CASES passed as shifts through W: mean,
    variance and conditional correlation of ndtri(u_out) within 5 standard errors, the Kolmogorov distance of
    Phi((ndtri(u) - mu) / s) within the DKW bound, and every row of out within it of the conditional CDF built from the
    long-double Fhat"""
    from mlmc_amd.tool import simple_distribution as sd
    worst, worst_x = np.zeros(4), 0.0
    for observed, z_obs in cc.STAT_CASES:
        w, fc, info = sd.conditional_factor(jc.CORR3, observed)
        mu = w @ np.array(z_obs)
        group = [table[0][m] for m in info.unobserved]
        out, u, _, _ = _cok(hip, group, fc, sc.DKW_N, shift=mu[None, :], first=first)
        stats = np.array(cc.score_statistics(special.ndtri(u[0]), mu, fc))
        worst = np.maximum(worst, stats)
        assert np.all(stats[:3] <= 5.0) and stats[3] <= sc.DKW_BOUND, (observed, stats)
        for p, row, m, s in zip(group, out[0], mu, info.s):
            f = qc.RuleTable(p["case"], p["lam"], p["quad"]).fhat(row)[0].astype(np.float64)
            cond = special.ndtr((special.ndtri(np.clip(f, U, 1.0 - U)) - m) / s)
            d = sc.kolmogorov_distance(cond)
            worst_x = max(worst_x, d)
            assert d <= sc.DKW_BOUND, (observed, p["tag"], d)
    print(f"\nfirst = {first}: mean {worst[0]:.3g}, variance {worst[1]:.3g}, correlation {worst[2]:.3g} standard errors, "
          f"Kolmogorov distances u {worst[3]:.4f} x {worst_x:.4f} (bound {sc.DKW_BOUND:.5f})")


def test_degenerate_problem(hip, table):
    """NaN multipliers in one problem among valid ones: its row is NaN in every set, its u_out and every z_out are still written,
    the other rows are bit-equal to a call without it; no error"""
    group = _cycle(table[0], 5)
    bad = dict(group[2])
    bad["lam"] = np.full_like(group[2]["lam"], np.nan)
    rng = np.random.default_rng(2)
    F = _scaled_factor(rng, 5, 5)
    shift = rng.uniform(-3.0, 3.0, (2, 5))
    want, want_u, want_z, want_mass = _cok(hip, group, F, 257, B=2, shift=shift, want_mass=True)
    for kind in (hip.HOST, hip.DEVICE):
        out, u, z, mass = _cok(hip, group[:2] + [bad] + group[3:], F, 257, B=2, shift=shift, kind=kind, want_mass=True)
        keep = [0, 1, 3, 4]
        assert np.all(np.isnan(out[:, 2])) and _same(out[:, keep], want[:, keep]) and _same(u, want_u) and _same(z, want_z)
        assert np.array_equal(mass[keep], want_mass[keep])


def test_errors_and_no_ops(hip, table):
    group = _cycle(table[0], 4)
    rng = np.random.default_rng(4)
    F = jc.random_factor(rng, 4, 3)
    shift = rng.uniform(-1.0, 1.0, (2, 4))

    def expect(rc, pattern):
        with pytest.raises(hip.MlmcHipError, match=pattern):
            hip.check(rc)
    assert _cond(hip, group, F, 2, B=2, shift=shift)[0] == 0
    expect(_cond(hip, group, F, -1)[0], NAME + ": n < 0")
    expect(_cond(hip, group, F, 2, first=-1)[0], NAME + ": first < 0")
    expect(_cond(hip, group, F, 2, first=2 ** 63 - 2)[0], NAME + ": first \\+ n overflows")
    assert _cond(hip, group, F, 2, first=2 ** 63 - 3)[0] == 0
    expect(_cond(hip, group, F, 2, kind=5)[0], NAME + ": bad mem_kind")
    expect(_cond(hip, group, F, 2, flags=2)[0], NAME + ": unknown flag")
    # the norm of a row: at most 1 within 1e-6, anything below is accepted
    bad = F.copy()
    bad[2] *= np.sqrt(1.0 + 1e-5)
    expect(_cond(hip, group, bad, 2)[0], NAME + ": factor row 2.*sum of squares")
    for scale in (np.sqrt(1.0 + 1e-7), np.sqrt(0.3), 0.0):
        ok = F.copy()
        ok[1] *= scale
        assert _cond(hip, group, ok, 2)[0] == 0, scale
    for value in (np.nan, np.inf):
        bad = F.copy()
        bad[3, 1] = value
        expect(_cond(hip, group, bad, 2)[0], NAME + ": factor row 3.*not finite")
        bad = shift.copy()
        bad[1, 2] = value
        expect(_cond(hip, group, F, 2, B=2, shift=bad)[0], NAME + ": shift of set 1, row 2")
    expect(_cond(hip, group, F, 2, B=0)[0], NAME + ": B < 1")
    expect(_cond(hip, group, F, 2, B=-3)[0], NAME + ": B < 1")
    for rows in ([0, 1, 1, 2], [0, 2, 1, 3], [-1, 0, 1, 2], [0, 1, 2, 6]):
        expect(_cond(hip, group, F, 2, rows=rows, ld_rows=6)[0], NAME + ": rows must be strictly increasing")
    expect(_cond(hip, group, F, 2, ld_rows=3)[0], NAME + ": ld_rows < M")
    # too many rows for a block of 64 draws: 192 MiB / (8 * 64) = 393216 rows with the normals; rejected before anything is read
    many = 400000
    lib, P = hip.lib(), hip.ptr
    handles, r1, lam, sig = _raw_args(hip, group[:1])
    a = np.array([group[0]["case"].domain[0]])
    b = np.array([group[0]["case"].domain[1]])
    quad = group[0]["quad"]
    one, out = np.array([[1.0]]), np.full((1, 2), SENTINEL)

    def raw(M=1, h=handles, B=1, shift=None, K=1, F=one, n=2, out=out, mass=None, quad=quad, b=b):
        return lib.mlmc_density_sample_conditional_batch(M, C.cast(h, C.c_void_p), P(r1), P(lam), P(sig), P(a), P(b), quad[0], quad[1], K,
                                                         P(F), 1, None, 0, n, 0, B, P(shift), None, max(M, 1), P(out), None, None, P(mass),
                                                         hip.HOST)
    assert raw() == 0
    expect(raw(B=many, shift=np.zeros(many)), NAME + ".*split the sets across calls")
    assert np.all(out != SENTINEL)
    expect(raw(K=0), NAME + ": K < 1")
    expect(raw(F=None), NAME + ": null factor")
    expect(raw(out=None), NAME + ".*null")
    expect(raw(M=-1), NAME + ".*M < 0")
    expect(raw(quad=(-1, 21)), NAME + ".*n_intervals")
    expect(raw(quad=(64, 65)), NAME + ".*gauss_degree")
    null_h = (C.c_void_p * 1)(None)
    expect(raw(h=null_h), NAME + ": problem 0.*null basis")
    expect(raw(b=a), NAME + ": problem 0.*domain")
    # no-ops: M = 0, and n = 0 (the arrays may be NULL then and are not touched; the masses are still returned)
    assert lib.mlmc_density_sample_conditional_batch(0, None, None, None, None, None, None, 0, 0, 0, None, 1, None, 0, 5, 0, 1, None, None,
                                                     0, None, None, None, None, hip.HOST) == 0
    out[:] = SENTINEL
    assert raw(n=0) == 0 and raw(n=0, out=None) == 0 and np.all(out == SENTINEL)
    mass = np.full(1, -1.0)
    assert raw(n=0, out=None, mass=mass) == 0
    assert np.array_equal(mass, _quantiles_c(hip, group[:1], quad, np.zeros(0), [0])[1]) and mass[0] > 0


@pytest.fixture(scope="module")
def marginals(table):
    """three marginals on the second rule whose quantiles resolve to the last bits (not the shifted case, whose x has a spacing of
    1e-13 on a domain of width 1e-2), and given values at fixed quantiles of the first"""
    group = [table[1][i] for i in (0, 2, 4)]
    return group, [p["dist"] for p in group]


def test_conditional_samples(hip, table, marginals):
    """conditional_samples == the C entry with conditional_factor's W and F_c and normal_scores' scores; observed rows hold the given
    values; an empty given == joint_samples; device tensors hold the same bits; shapes; an out-of-domain value raises"""
    import torch
    from mlmc_amd.tool import simple_distribution as sd
    group, distrs = marginals
    n = 257
    x1 = sd.quantiles([distrs[1]], [np.array([0.2, 0.5, 0.93, 0.5])])[0]
    given = {1: x1}
    w, fc, info = sd.conditional_factor(jc.CORR3, [1])
    z_obs, u_obs = sd.normal_scores([distrs[1]], x1[None, :], return_uniforms=True)
    mu = np.ascontiguousarray((w @ z_obs).T)
    want, want_u, _, _ = _cok(hip, [group[0], group[2]], fc, n, B=4, shift=mu, first=3, flags=1)
    x, u = sd.conditional_samples(distrs, n, SEED, given, corr=jc.CORR3, first=3, antithetic=True, return_uniforms=True)
    assert x.shape == (4, 3, n) and _same(x[:, [0, 2]], want) and _same(u[:, [0, 2]], want_u)
    assert np.array_equal(x[:, 1], np.tile(x1[:, None], (1, n))) and np.array_equal(u[:, 1], np.tile(u_obs[0][:, None], (1, n)))
    assert _same(x[3], x[1]) and not _same(x[0], x[1])
    assert _same(sd.conditional_samples(distrs, n, SEED, given, factor_info=(w, fc, info), first=3, antithetic=True), x)
    xd, ud = sd.conditional_samples(distrs, n, SEED, given, corr=jc.CORR3, first=3, antithetic=True, device=True, return_uniforms=True)
    for d, ref in ((xd, x), (ud, u)):
        assert isinstance(d, torch.Tensor) and d.is_cuda and d.dtype == torch.float64 and _same(d.cpu().numpy(), ref)
    # scalars: [M, n], equal to the set among four; two given components, one of them an array
    xs = sd.conditional_samples(distrs, n, SEED, {1: float(x1[2])}, corr=jc.CORR3, first=3, antithetic=True)
    assert xs.shape == (3, n) and _same(xs, x[2])
    x0 = float(sd.quantiles([distrs[0]], [np.array([0.7])])[0][0])
    both = sd.conditional_samples(distrs, 64, SEED, {1: x1[:2], 0: x0}, corr=jc.CORR3)
    assert both.shape == (2, 3, 64) and np.all(both[:, 0] == x0) and np.array_equal(both[:, 1], np.tile(x1[:2, None], (1, 64)))
    assert np.all((both[:, 2] >= distrs[2].domain[0]) & (both[:, 2] <= distrs[2].domain[1]))
    # an empty given: joint_samples bit for bit
    xj, uj = sd.joint_samples(distrs, n, SEED, corr=jc.CORR3, first=3, antithetic=True, return_uniforms=True)
    xe, ue = sd.conditional_samples(distrs, n, SEED, {}, corr=jc.CORR3, first=3, antithetic=True, return_uniforms=True)
    assert _same(xe, xj) and _same(ue, uj)
    assert sd.conditional_samples(distrs, 0, SEED, given, corr=jc.CORR3).shape == (4, 3, 0)
    # a value outside the open domain, NaN: the error names component and set
    bad = x1.copy()
    bad[2] = distrs[1].domain[1]
    with pytest.raises(ValueError, match=r"component 1 \(set 2\)"):
        sd.conditional_samples(distrs, 4, SEED, {1: bad}, corr=jc.CORR3)
    with pytest.raises(ValueError, match=r"component 0 \(set 0\)"):
        sd.conditional_samples(distrs, 4, SEED, {0: np.nan}, corr=jc.CORR3)
    with pytest.raises(ValueError, match="exactly one of corr"):
        sd.conditional_samples(distrs, 4, SEED, given)
    with pytest.raises(ValueError, match="does not belong"):
        sd.conditional_samples(distrs, 4, SEED, {0: x0}, factor_info=(w, fc, info))
    mixed = [distrs[0], table[0][1]["dist"], distrs[2]]
    with pytest.raises(ValueError, match="same quadrature"):
        sd.conditional_samples(mixed, 4, SEED, {}, corr=jc.CORR3)


def test_conditional_quantiles_and_cdfs(hip, marginals):
    """conditional_quantiles == quantiles at the host-mapped p' bit for bit; the end points and what is no probability;
    conditional_cdfs(conditional_quantiles(p)) returns p; the empirical CDF of 16384 conditional draws lies within the DKW bound
    of conditional_cdfs"""
    from mlmc_amd.tool import simple_distribution as sd
    group, distrs = marginals
    x1 = sd.quantiles([distrs[1]], [np.array([0.2, 0.5, 0.93])])[0]
    given = {1: x1}
    w, fc, info = sd.conditional_factor(jc.CORR3, [1])
    z_obs = sd.normal_scores([distrs[1]], x1[None, :])
    mu = (w @ z_obs).T                                                        # [B, q]
    probs = np.array([0.0, 0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 1.0, np.nan, -0.1, 1.1])
    q = sd.conditional_quantiles(distrs, probs, given, jc.CORR3)
    assert q.shape == (3, 2, probs.size)
    with np.errstate(invalid="ignore"):
        mapped = special.ndtr(mu[:, :, None] + info.s[None, :, None] * special.ndtri(probs)[None, None, :])
    free = [distrs[0], distrs[2]]
    want = sd.quantiles(free, [mapped[:, m].ravel() for m in range(2)])
    for m in range(2):
        assert _same(q[:, m].ravel(), want[m]), m
        assert np.all(q[:, m, 0] == free[m].domain[0]) and np.all(q[:, m, 8] == free[m].domain[1]) and np.all(np.isnan(q[:, m, 9:]))
        assert np.all(np.diff(q[:, m, :9], axis=1) > 0)
    qs = sd.conditional_quantiles(distrs, probs, {1: float(x1[1])}, jc.CORR3)
    assert qs.shape == (2, probs.size) and _same(qs, q[1])
    # the round trip on the inner probabilities, in units of 2^-53; for comparison the long-double Fhat pushed through the same map
    inner = slice(1, 8)
    back = sd.conditional_cdfs(distrs, q[:, :, inner], given, jc.CORR3)
    assert back.shape == (3, 2, 7)
    units = np.abs(back - probs[inner][None, None, :]) / U
    ref_units = np.zeros_like(units)
    for m, p in enumerate((group[0], group[2])):
        f = qc.RuleTable(p["case"], p["lam"], p["quad"]).fhat(q[:, m, inner].ravel())[0].astype(np.float64).reshape(3, 7)
        ref = special.ndtr((special.ndtri(np.clip(f, U, 1.0 - U)) - mu[:, m, None]) / info.s[m])
        ref_units[:, m] = np.abs(ref - probs[inner][None, :]) / U
    print(f"\nconditional_cdfs(conditional_quantiles(p)) - p: worst {units.max():.4g} units of 2^-53 (the long-double Fhat through the "
          f"same map: {ref_units.max():.4g}; recorded {cc.ROUNDTRIP_UNITS_OBSERVED}, tolerance "
          f"{jc.tolerance(cc.ROUNDTRIP_UNITS_OBSERVED):g})")
    assert units.max() <= jc.tolerance(cc.ROUNDTRIP_UNITS_OBSERVED)
    assert _same(sd.conditional_cdfs(distrs, q[1, :, inner], {1: float(x1[1])}, jc.CORR3), back[1])
    # the draws of one component against its conditional CDF
    draws = sd.conditional_samples(distrs, sc.DKW_N, SEED, {1: float(x1[2])}, corr=jc.CORR3)
    cdf = sd.conditional_cdfs(distrs, draws[2], {1: float(x1[2])}, jc.CORR3)
    assert cdf.shape == (2, sc.DKW_N)
    d = sc.kolmogorov_distance(cdf[1])
    print(f"Kolmogorov distance of 16384 conditional draws from conditional_cdfs: {d:.4f} (bound {sc.DKW_BOUND:.5f})")
    assert d <= sc.DKW_BOUND


def test_estimate_conditional(hip):
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
    n = 500
    before, _, used = est.sample_joint(n, SEED, densities=pdfs)
    mid = [0.5 * (doms[m][0] + doms[m][1]) for m in range(M)]
    given = {1: mid[1], 3: np.array([mid[3], 0.7 * doms[3][0] + 0.3 * doms[3][1]])}
    draws, ok, info = est.sample_conditional(n, SEED, given, densities=pdfs)
    assert draws.shape == (2, M, n) and ok.shape == (M,) and np.array_equal(ok, np.array([bool(d[2].success) for d in pdfs]))
    assert type(info).__name__ == "ConditionalFactorInfo" and info.unobserved.tolist() == [0, 2] and np.all((info.s > 0) & (info.s <= 1 + 4 * U))
    cov, _ = est.estimate_component_covariance()
    s = np.sqrt(np.diag(cov))
    corr = cov / s[:, None] / s[None, :]
    np.fill_diagonal(corr, 1.0)
    cond = sd.conditional_factor(corr, [1, 3])
    assert _same(draws, sd.conditional_samples(distrs, n, SEED, given, factor_info=cond))
    assert _same(draws, sd.conditional_samples(distrs, n, SEED, given, corr=corr))
    assert np.all(draws[:, 1] == mid[1]) and np.all(draws[0, 3] == given[3][0]) and np.all(draws[1, 3] == given[3][1])
    for m in (0, 2):
        assert np.all((draws[:, m] >= doms[m][0]) & (draws[:, m] <= doms[m][1]))
    fresh, ok2, info2 = est.sample_conditional(n, SEED, given, tol=1e-8, orth_moments_tol=1e-4, moments_fns=fns)
    assert _same(fresh, draws) and np.array_equal(ok2, ok) and np.array_equal(info2.s, info.s)
    on_dev, _, _ = est.sample_conditional(n, SEED, given, densities=pdfs, device=True)
    assert isinstance(on_dev, torch.Tensor) and on_dev.is_cuda and on_dev.shape == (2, M, n) and _same(on_dev.cpu().numpy(), draws)
    # corr = "scores" and a matrix
    by_scores, _, _ = est.sample_conditional(n, SEED, {1: mid[1]}, corr="scores", densities=pdfs)
    score_corr = est.estimate_score_correlation(densities=pdfs).corr
    by_matrix, _, info_m = est.sample_conditional(n, SEED, {1: mid[1]}, corr=score_corr, densities=pdfs)
    assert by_scores.shape == (M, n) and _same(by_scores, by_matrix) and info_m.unobserved.tolist() == [0, 2, 3]
    assert _same(by_matrix, sd.conditional_samples(distrs, n, SEED, {1: mid[1]}, corr=score_corr))
    cont, _, _ = est.sample_conditional(100, SEED, {1: mid[1]}, corr=score_corr, densities=pdfs, first=400, antithetic=True)
    assert _same(cont, sd.conditional_samples(distrs, 100, SEED, {1: mid[1]}, corr=score_corr, first=400, antithetic=True))
    # the quantiles: shape, monotone in p, inside each domain
    probs = np.array([0.05, 0.25, 0.5, 0.75, 0.95])
    cq, ok3 = est.estimate_conditional_quantiles(probs, {1: mid[1], 3: mid[3]}, densities=pdfs)
    assert cq.shape == (2, probs.size) and np.array_equal(ok3, ok) and np.all(np.diff(cq, axis=1) > 0)
    for row, m in zip(cq, (0, 2)):
        assert np.all((row > doms[m][0]) & (row < doms[m][1]))
    assert _same(cq, sd.conditional_quantiles(distrs, probs, {1: mid[1], 3: mid[3]}, corr))
    cq2, _ = est.estimate_conditional_quantiles(probs, given, corr="scores", densities=pdfs)
    assert cq2.shape == (2, 2, probs.size)
    # sample_joint afterwards returns what it returned before
    after, _, used2 = est.sample_joint(n, SEED, densities=pdfs)
    assert _same(after, before) and np.array_equal(used2, used)
    with pytest.raises(ValueError, match="n must be"):
        est.sample_conditional(-1, SEED, given, densities=pdfs)
    with pytest.raises(ValueError, match="corr must be"):
        est.sample_conditional(4, SEED, given, corr="pearson", densities=pdfs)
