"""GPU tests of the conditional joint draws under the Student-t copula (the SHIFT and TSCALE instance of k_cop_uniforms in
mlmc_amd/csrc/copula.hip, k_cop_mixing / k_tcop_map of copula_t.hip with the constants of nu_c and nu, q_copula with sets and a t
copula in density.hip) through mlmc_density_sample_conditional_t_batch and mlmc_chi2_conditional_scale,
simple_distribution.conditional_samples / conditional_quantiles / conditional_cdfs with dof and the two Estimate methods.

x[b][m][j] = Q_m(u), u = clamp(T_nu(y)), y = shift[b][m] (+) ((acc (x) s[j]) (x) scale[b]) (include/mlmc_hip.h).  With a zero shift,
unit scales and dof_mix = dof the entry is compared bit for bit with the joint t entry, the epilogue with mpmath at the device's
own normals and mixing scales, the structure bit for bit, the law with counts against conditional_quantiles."""
import ctypes as C

import numpy as np
import pytest
from scipy import special

from tests import conditional_t_cases as ct
from tests import joint_sample_cases as jc
from tests import t_copula_cases as tc
from tests.test_gpu_density_samples import SEED, _quantiles_c, _same
from tests.test_gpu_quantiles import _raw_args
from tests.test_gpu_t_copula import ANTITHETIC, SOBOL, _cycle, _entry, _last_error, _mp_t_cdf_ld, _scale, _t_cdf, group6, hip  # noqa: F401
from tests.test_gpu_t_copula import _ok as _joint_t_ok

pytestmark = pytest.mark.gpu
NAME = "mlmc_density_sample_conditional_t_batch"
U = jc.U
SENTINEL = 7.25


def _tcond(hip, group, F, n, dof, dof_mix=None, B=1, shift=None, scale=None, rows=None, ld_rows=None, seed=SEED, streams=None,
           mix_stream=None, first=0, flags=0, kind=None, want_u=True, want_z=True, want_s=True, want_mass=False):
    """mlmc_density_sample_conditional_t_batch on the problems of `group`; returns (rc, out [B, ld_rows, n], u [B, ld_rows, n],
    z [K, n], s [n], mass); the arrays are filled with SENTINEL before the call"""
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
    sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
    rw = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
    ld = M if ld_rows is None else ld_rows
    cols, sets, height = max(int(n), 0), max(int(B), 1), max(ld, M)
    mix_stream = K if mix_stream is None else mix_stream
    dof_mix = dof if dof_mix is None else dof_mix

    def array(shape, want):
        if not want:
            return None
        if kind == hip.DEVICE:
            return torch.full(shape, SENTINEL, dtype=torch.float64, device="cuda")
        return np.full(shape, SENTINEL)
    out, u = array((sets, height, cols), True), array((sets, height, cols), want_u)
    z, s = array((K, cols), want_z), array((cols,), want_s)
    if kind == hip.DEVICE:
        torch.cuda.synchronize()
    mass = np.full(M, -1.0) if want_mass else None
    quad = group[0]["quad"]
    rc = hip.lib().mlmc_density_sample_conditional_t_batch(
        M, C.cast(handles, C.c_void_p), hip.ptr(r1), hip.ptr(lam), hip.ptr(sig), hip.ptr(a), hip.ptr(b), quad[0], quad[1], K, hip.ptr(F),
        float(dof), float(dof_mix), seed, hip.ptr(st), mix_stream, first, n, flags, B, hip.ptr(sh), hip.ptr(sc), hip.ptr(rw), ld,
        hip.ptr(out), hip.ptr(u), hip.ptr(z), hip.ptr(s), hip.ptr(mass), kind)
    if kind == hip.DEVICE:
        out, u, z, s = (None if v is None else v.cpu().numpy() for v in (out, u, z, s))
    return rc, out, u, z, s, mass


def _tok(hip, *args, **kw):
    rc, out, u, z, s, mass = _tcond(hip, *args, **kw)
    hip.check(rc)
    return out, u, z, s, mass


def _cscale(hip, dof_mix, p, kind=None):
    rc, out = _entry(hip, "mlmc_chi2_conditional_scale", dof_mix, p, kind)
    hip.check(rc)
    return out


def _scaled_factor(rng, M, K):
    """random rows scaled by factors in [0, 1]: row M // 2 exactly zero, row 0 of norm 1"""
    F = jc.random_factor(rng, M, K) * rng.uniform(0.0, 1.0, M)[:, None]
    F[M // 2] = 0.0
    if M > 1:
        F[0] = jc.random_factor(rng, 1, K)[0]
    return np.ascontiguousarray(F)


# ---- reduction to the joint t entry ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,K,n,first", ct.REDUCTION_SHAPES)
def test_reduction_to_the_joint_t_entry(hip, group6, M, K, n, first):
    """B = 1, a NULL shift and scale or explicit zeros and ones, dof_mix == dof, unit rows: out, u_out, z_out and s_out are the
    joint t entry's bits; host and device arrays, antithetic, Sobol'"""
    group = _cycle(group6, M)
    F = jc.random_factor(np.random.default_rng(100 * M + K), M, K)
    for dof in ct.REDUCTION_DOFS:
        want = _joint_t_ok(hip, group, F, n, dof, first=first)
        for shift, scale in ((None, None), (np.zeros((1, M)), np.ones(1))):
            for kind in (hip.HOST, hip.DEVICE):
                out, u, z, s, _ = _tok(hip, group, F, n, dof, first=first, shift=shift, scale=scale, kind=kind)
                assert _same(out[0], want[0]) and _same(u[0], want[1]) and _same(z, want[2]) and _same(s, want[3]), (dof, kind)
        for flags in (ANTITHETIC, SOBOL):
            want = _joint_t_ok(hip, group, F, n, dof, first=first, flags=flags)
            out, u, z, s, _ = _tok(hip, group, F, n, dof, first=first, flags=flags)
            assert _same(out[0], want[0]) and _same(u[0], want[1]) and _same(z, want[2]) and _same(s, want[3]), (dof, flags)


# ---- the epilogue ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dof,dof_mix", ct.EPILOGUE_DOFS)
@pytest.mark.parametrize("M,K,n,B", ct.EPILOGUE_SHAPES)
def test_epilogue(hip, group6, M, K, n, B, dof, dof_mix):
    """rows of F scaled into [0, 1] (one exactly zero), shifts in [-3, 3], scales in [0.3, 3]: u_out against T_nu (mpmath) of
    shift + scale s (the long-double dot of F with the device's own z_out) at the device's own s_out, within
        t_nu(y) ((K + 4) 2^-53 r s sum_k |F_mk z_k| + 2^-53 |y|) + E_T 2^-53 max(T, 2^-53):
    the chain's error and the two rounded multiplications scaled by r s, the rounded addition, and the error of the t CDF"""
    rng = np.random.default_rng(1000 * M + 10 * K + B)
    F = _scaled_factor(rng, M, K) if M > 1 else np.array([[0.6]])
    shift = rng.uniform(-3.0, 3.0, (B, M))
    scale = rng.uniform(0.3, 3.0, B)
    _, u, z, s, _ = _tok(hip, _cycle(group6, M), F, n, dof, dof_mix, B=B, shift=shift, scale=scale)
    assert np.all((u >= jc.U_LO) & (u <= jc.U_HI)) and np.all(np.isfinite(s) & (s > 0))
    dot = jc.ld_dot(F, z) * s.astype(jc.LD)[None, :]
    absdot = (np.abs(F) @ np.abs(z)) * s[None, :]
    worst = 0.0
    for b in range(B):
        y = shift[b].astype(jc.LD)[:, None] + jc.LD(scale[b]) * dot
        ref_mp = _mp_t_cdf_ld(dof, y)
        ref = np.array([float(v) for v in ref_mp]).reshape(M, n)
        err = jc.phi_abs_errors(u[b], ref_mp).reshape(M, n)
        yd = y.astype(np.float64)
        dens = np.exp(special.gammaln(0.5 * (dof + 1.0)) - special.gammaln(0.5 * dof)) / np.sqrt(dof * np.pi) \
            * (1.0 + yd * yd / dof) ** (-0.5 * (dof + 1.0))
        bound = dens * ((K + 4) * U * scale[b] * absdot + U * np.abs(yd)) + jc.tolerance(tc.T_UNITS_OBSERVED) * U * np.maximum(ref, U)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (b, float(np.max(err / bound)))
    print(f"\nM {M} K {K} n {n} B {B} nu {dof:g} nu_c {dof_mix:g}: worst error / bound {worst:.3g}")


# ---- structure -------------------------------------------------------------------------------------------------------------------

def test_exact_structure(hip, group6, monkeypatch):
    """a zero row, equal (shift, scale), a scale alone, a set alone against the set among five, a permutation of the sets,
    rows / ld_rows, first / n, the block length"""
    rng = np.random.default_rng(21)
    M, K, n, B = ct.STRUCTURE_SHAPE
    dof, dof_mix = 3.0, 5.0
    group = _cycle(group6, M)
    quad = group[0]["quad"]
    F = _scaled_factor(rng, M, K)
    shift = rng.uniform(-3.0, 3.0, (B, M))
    scale = rng.uniform(0.3, 3.0, B)
    shift[3], scale[3] = shift[1], scale[1]                                # two sets with equal shift and scale
    shift[4] = shift[0]                                                    # two sets that differ in the scale alone
    assert scale[4] != scale[0]
    out, u, z, s, _ = _tok(hip, group, F, n, dof, dof_mix, B=B, shift=shift, scale=scale)
    zero = M // 2
    assert np.all(F[zero] == 0.0)
    for b in range(B):
        assert np.all(u[b, zero] == u[b, zero, 0]) and np.all(out[b, zero] == out[b, zero, 0])
        ref = tc.mp_t_cdf(dof, [shift[b, zero]])
        assert tc.t_units(u[b, zero, :1], ref)[0] <= jc.tolerance(tc.T_UNITS_OBSERVED)
        assert u[b, zero, 0] == tc.clamp(_t_cdf(hip, dof, [shift[b, zero]]))[0]
        want, _ = _quantiles_c(hip, [group[zero]], quad, u[b, zero, :1], [1])
        assert out[b, zero, 0] == want[0]
    assert _same(out[3], out[1]) and _same(u[3], u[1]) and not _same(u[0], u[1])
    live = [m for m in range(M) if m != zero]
    assert _same(u[4, zero], u[0, zero]) and all(not _same(u[4, m], u[0, m]) for m in live)
    for b in (0, 2, 4):
        alone = _tok(hip, group, F, n, dof, dof_mix, B=1, shift=shift[b:b + 1], scale=scale[b:b + 1])
        assert _same(alone[0][0], out[b]) and _same(alone[1][0], u[b]) and _same(alone[2], z) and _same(alone[3], s), b
    perm = np.array([4, 0, 3, 1, 2])
    for kind in (hip.HOST, hip.DEVICE):
        got = _tok(hip, group, F, n, dof, dof_mix, B=B, shift=shift[perm], scale=scale[perm], kind=kind)
        assert _same(got[0], out[perm]) and _same(got[1], u[perm]) and _same(got[2], z) and _same(got[3], s), kind
    # rows = [1, 3, 4] of 6: the named rows are the identity layout's rows, the others keep the sentinel
    sub, Fs, shs = group[:3], F[:3], shift[:, :3]
    ident = _tok(hip, sub, Fs, n, dof, dof_mix, B=B, shift=shs, scale=scale)
    assert _same(ident[0], out[:, :3]) and _same(ident[1], u[:, :3])          # no value depends on M (mix_stream aside)
    for kind in (hip.HOST, hip.DEVICE):
        for want_u in (True, False):
            got = _tok(hip, sub, Fs, n, dof, dof_mix, B=B, shift=shs, scale=scale, rows=[1, 3, 4], ld_rows=6, kind=kind, want_u=want_u)
            arrays = ((got[0], ident[0]), (got[1], ident[1])) if want_u else ((got[0], ident[0]),)
            for g, w in arrays:
                assert g.shape == (B, 6, n) and _same(g[:, [1, 3, 4]], w) and np.all(g[:, [0, 2, 5]] == SENTINEL), (kind, want_u)
            assert _same(got[2], ident[2]) and _same(got[3], ident[3])
    # first = 50, n = 100 gives columns [50, 150) of first = 0, n = 150
    whole = _tok(hip, group, F, 150, dof, dof_mix, B=B, shift=shift, scale=scale)
    part = _tok(hip, group, F, 100, dof, dof_mix, B=B, shift=shift, scale=scale, first=50)
    assert _same(part[0], whole[0][:, :, 50:]) and _same(part[1], whole[1][:, :, 50:]) and _same(part[2], whole[2][:, 50:])
    assert _same(part[3], whole[3][50:]) and _same(whole[0], out[:, :, :150])
    # blocks of 64 draws (64 + 64 + 64 + 64 + 1)
    monkeypatch.setenv("MLMC_JOINT_BLOCK_DRAWS", "64")
    for kind in (hip.HOST, hip.DEVICE):
        got = _tok(hip, group, F, n, dof, dof_mix, B=B, shift=shift, scale=scale, kind=kind)
        assert _same(got[0], out) and _same(got[1], u) and _same(got[2], z) and _same(got[3], s), kind
        bare = _tok(hip, group, F, n, dof, dof_mix, B=B, shift=shift, scale=scale, kind=kind, want_u=False, want_z=False, want_s=False)
        assert _same(bare[0], out), kind


# ---- the mixing scale ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, ANTITHETIC, SOBOL])
def test_mixing_scales_of_the_entry(hip, group6, flags):
    """s_out == mlmc_chi2_conditional_scale(dof_mix) at the host restatement of the mixing uniform, bit for bit"""
    group, F = _cycle(group6, 3), _scaled_factor(np.random.default_rng(3), 3, 2)
    for first in (0, 50):
        for dof, dof_mix, mix_stream in ((3.0, 4.0, 2), (30.0, 33.0, 977), (64.0, 192.0, 5)):
            _, _, z, s, _ = _tok(hip, group, F, 130, dof, dof_mix, B=2, shift=np.zeros((2, 3)), scale=[1.0, 2.0], mix_stream=mix_stream,
                                 first=first, flags=flags)
            p0 = tc.mixing_uniforms(SEED, mix_stream, first, 130, antithetic=flags == ANTITHETIC, qmc=flags == SOBOL)
            assert _same(s, _cscale(hip, dof_mix, p0)), (flags, first, dof_mix)
            if flags == ANTITHETIC:
                assert _same(s[0::2], s[1::2]) and _same(z[:, 0::2], -z[:, 1::2])


def test_conditional_scale_up_to_64_is_the_mixing_scale(hip):
    p = tc.p_arguments()
    for dof in tc.DOFS:
        want = _scale(hip, dof, p)
        assert _same(_cscale(hip, dof, p), want) and _same(_cscale(hip, dof, p, hip.DEVICE), want), dof


@pytest.mark.parametrize("dof_mix", ct.WIDE_DOFS)
def test_conditional_scale_beyond_64(hip, dof_mix):
    """finite and positive over p_arguments(), within tolerance(the twin's record) of mpmath in s_units"""
    p = tc.p_arguments()
    s = _cscale(hip, dof_mix, p)
    assert np.all(np.isfinite(s) & (s > 0.0))
    units = tc.s_units(dof_mix, p, s)
    k = int(np.argmax(units))
    gate = jc.tolerance(max(ct.S_UNITS_OBSERVED_TWIN_WIDE.values()))
    print(f"\nnu_c {dof_mix:g}: chi2 conditional scale worst {units[k]:.4g} units at p = {p[k]!r} (the twin: "
          f"{ct.S_UNITS_OBSERVED_TWIN_WIDE[dof_mix]}, tolerance {gate:g})")
    assert units[k] <= gate
    assert np.all(np.isnan(_cscale(hip, dof_mix, [0.0, 1.0, -0.25, 1.5, np.nan])))


# ---- the law ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def marginals(group6):
    """three marginals whose quantiles resolve to the last bits (not the shifted case, whose x has a spacing of 1e-13 on a domain
    of width 1e-2)"""
    group = [group6[i] for i in (0, 2, 4)]
    return group, [p["dist"] for p in group]


def test_the_law_statistically(hip, marginals):
    """M = 3 at jc.CORR3, component 0 given at its median and at its 0.999-quantile, nu = 3, 2^16 draws: for each free component
    and p in (0.05, 0.5, 0.95) the share of draws below conditional_quantiles(p, dof=3) lies within 5 binomial standard errors
    of p; the 90 % band of the far set is wider than that of the median set by the ratio of their r, in the quantiles exactly and in
    the draws within 5 standard errors of the empirical quantiles; under dof=None the two bands have equal width in score space"""
    from mlmc_amd.tool import simple_distribution as sd
    _, distrs = marginals
    dof, n = ct.STAT_DOF, ct.STAT_N
    probs = np.array(ct.STAT_PROBS)
    x0 = sd.quantiles([distrs[0]], [np.array([0.5, ct.STAT_FAR])])[0]
    given = {0: x0}
    x, u = sd.conditional_samples(distrs, n, SEED, given, corr=jc.CORR3, dof=dof, return_uniforms=True)
    q = sd.conditional_quantiles(distrs, probs, given, jc.CORR3, dof=dof)                       # [2, 2, 3]
    assert x.shape == (2, 3, n) and q.shape == (2, 2, 3)
    worst = 0.0
    for b in range(2):
        for i, m in enumerate((1, 2)):
            for k, p in enumerate(probs):
                share = np.mean(x[b, m] < q[b, i, k])
                worst = max(worst, abs(share - p) / np.sqrt(p * (1 - p) / n))
                assert abs(share - p) <= 5.0 * np.sqrt(p * (1 - p) / n), (b, m, p, share)
    # the conditional scales of the two sets, from the same matrix
    w, _, info, l_oo = sd.conditional_factor(jc.CORR3, [0], return_observed=True)
    y_obs = sd.t_scores(sd.normal_scores([distrs[0]], x0[None, :]), dof)
    r = sd._conditional_t_scale(y_obs, l_oo, dof)
    ratio = r[1] / r[0]
    assert ratio > 3.0                                                                      # an extreme value widens the law
    tq = special.stdtrit(dof + 1.0, probs[[0, 2]])
    for i, m in enumerate((1, 2)):
        # the quantiles: the t scores of the band's ends are mu + r s T^-1(p), so the widths are in the ratio of the r
        yq = sd._t_quantile_lower_tail(sd.cdfs_on_rule([distrs[m]], [q[:, i, [0, 2]].ravel()])[0], dof).reshape(2, 2)
        width_q = yq[:, 1] - yq[:, 0]
        assert abs(width_q[1] / width_q[0] / ratio - 1.0) <= 1e-8, (m, width_q, ratio)
        # the draws: empirical 5 % and 95 % quantiles of the t scores; the standard error of a sample quantile is
        # sqrt(p (1 - p) / n) / density, the density of the conditional law being t_{nu + 1}((y - mu) / (r s)) / (r s)
        y = np.sort(sd._t_quantile_lower_tail(u[:, m], dof), axis=1)
        width = y[:, int(0.95 * n)] - y[:, int(0.05 * n)]
        dens = special.gamma(0.5 * (dof + 2.0)) / (np.sqrt((dof + 1.0) * np.pi) * special.gamma(0.5 * (dof + 1.0))) \
            * (1.0 + tq[0] ** 2 / (dof + 1.0)) ** (-0.5 * (dof + 2.0))
        se_width = np.sqrt(2.0 * 0.05 * 0.95 / n) / (dens / (r * info.s[i]))                  # [2]
        rel = np.sqrt(np.sum((se_width / width) ** 2))
        print(f"\ncomponent {m}: band ratio far / median {width[1] / width[0]:.4f} in the draws, {ratio:.4f} = r_far / r_median "
              f"({abs(width[1] / width[0] / ratio - 1.0) / rel:.2f} standard errors)")
        assert abs(width[1] / width[0] / ratio - 1.0) <= 5.0 * rel
    print(f"worst share: {worst:.2f} binomial standard errors")
    # the Gaussian copula: the same spread whatever was observed
    _, ug = sd.conditional_samples(distrs, n, SEED, given, corr=jc.CORR3, return_uniforms=True)
    zg = np.sort(special.ndtri(ug[:, 1:]), axis=2)
    wg = zg[:, :, int(0.95 * n)] - zg[:, :, int(0.05 * n)]
    assert np.max(np.abs(wg[1] - wg[0])) <= 1e-9


# ---- the Python entries ------------------------------------------------------------------------------------------------------------

def test_python_entries(hip, marginals):
    import torch
    from mlmc_amd.tool import simple_distribution as sd
    group, distrs = marginals
    n, dof = 257, 3.0
    x1 = sd.quantiles([distrs[1]], [np.array([0.2, 0.5, 0.93, 0.5])])[0]
    given = {1: x1}
    # the C entry with conditional_factor's W, F_c and L_OO, the t scores of normal_scores' scores and the conditional scale
    w, fc, info, l_oo = sd.conditional_factor(jc.CORR3, [1], return_observed=True)
    z_obs, u_obs = sd.normal_scores([distrs[1]], x1[None, :], return_uniforms=True)
    y_obs = sd.t_scores(z_obs, dof)
    mu, r = np.ascontiguousarray((w @ y_obs).T), sd._conditional_t_scale(y_obs, l_oo, dof)
    want = _tok(hip, [group[0], group[2]], fc, n, dof, dof + 1.0, B=4, shift=mu, scale=r, first=3, flags=ANTITHETIC)
    x, u, s = sd.conditional_samples(distrs, n, SEED, given, corr=jc.CORR3, first=3, antithetic=True, dof=dof, return_uniforms=True,
                                     return_mixing=True)
    assert x.shape == (4, 3, n) and s.shape == (n,)
    assert _same(x[:, [0, 2]], want[0]) and _same(u[:, [0, 2]], want[1]) and _same(s, want[3])
    assert np.array_equal(x[:, 1], np.tile(x1[:, None], (1, n))) and np.array_equal(u[:, 1], np.tile(u_obs[0][:, None], (1, n)))
    assert _same(x[3], x[1]) and not _same(x[0], x[1])
    assert _same(sd.conditional_samples(distrs, n, SEED, given, factor_info=(w, fc, info, l_oo), first=3, antithetic=True, dof=dof), x)
    xs, ss = sd.conditional_samples(distrs, n, SEED, given, corr=jc.CORR3, first=3, antithetic=True, dof=dof, return_mixing=True)
    assert _same(xs, x) and _same(ss, s)
    xd, ud, sdev = sd.conditional_samples(distrs, n, SEED, given, corr=jc.CORR3, first=3, antithetic=True, dof=dof, device=True,
                                          return_uniforms=True, return_mixing=True)
    for d, ref in ((xd, x), (ud, u), (sdev, s)):
        assert isinstance(d, torch.Tensor) and d.is_cuda and d.dtype == torch.float64 and _same(d.cpu().numpy(), ref)
    # explicit streams and a mixing stream of one's own; qmc
    a = sd.conditional_samples(distrs, 64, SEED, given, corr=jc.CORR3, dof=dof, streams=[0, 1], mix_stream=2)
    assert _same(a, sd.conditional_samples(distrs, 64, SEED, given, corr=jc.CORR3, dof=dof))
    assert not _same(a, sd.conditional_samples(distrs, 64, SEED, given, corr=jc.CORR3, dof=dof, streams=[0, 1], mix_stream=9))
    assert sd.conditional_samples(distrs, 64, SEED, given, corr=jc.CORR3, dof=dof, qmc=True).shape == (4, 3, 64)
    # scalars: [M, n], equal to the set among four
    scal = sd.conditional_samples(distrs, n, SEED, {1: float(x1[2])}, corr=jc.CORR3, first=3, antithetic=True, dof=dof)
    assert scal.shape == (3, n) and _same(scal, x[2])
    # None and inf: the Gaussian results bit for bit
    gx, gu = sd.conditional_samples(distrs, n, SEED, given, corr=jc.CORR3, first=3, return_uniforms=True)
    for none in (None, np.inf):
        hx, hu = sd.conditional_samples(distrs, n, SEED, given, corr=jc.CORR3, first=3, return_uniforms=True, dof=none)
        assert _same(hx, gx) and _same(hu, gu)
    assert not _same(gx, sd.conditional_samples(distrs, n, SEED, given, corr=jc.CORR3, first=3, dof=dof))
    # an empty given: joint_samples(dof=...) bit for bit
    xj, uj, sj = sd.joint_samples(distrs, n, SEED, corr=jc.CORR3, first=3, antithetic=True, dof=dof, return_uniforms=True, return_mixing=True)
    xe, ue, se = sd.conditional_samples(distrs, n, SEED, {}, corr=jc.CORR3, first=3, antithetic=True, dof=dof, return_uniforms=True,
                                        return_mixing=True)
    assert _same(xe, xj) and _same(ue, uj) and _same(se, sj)
    assert sd.conditional_samples(distrs, 0, SEED, given, corr=jc.CORR3, dof=dof).shape == (4, 3, 0)
    # the elementwise entry
    p = np.array([[0.01, 0.5], [0.99, 2.0 ** -53]])
    assert _same(sd.conditional_mixing_scale(p, 150.5).ravel(), _cscale(hip, 150.5, p.ravel()))
    assert _same(sd.conditional_mixing_scale(p, 30.0), sd.chi2_mixing_scale(p, 30.0))
    pd = sd.conditional_mixing_scale(torch.from_numpy(p).cuda(), 150.5, device=True)
    assert pd.is_cuda and _same(pd.cpu().numpy(), sd.conditional_mixing_scale(p, 150.5))


def test_conditional_quantiles_and_cdfs(hip, marginals):
    """conditional_quantiles(dof) == quantiles at the host-mapped p' bit for bit; the round trip through conditional_cdfs returns p
    within the tolerance of the host maps; None and inf are the Gaussian results"""
    from mlmc_amd.tool import simple_distribution as sd
    _, distrs = marginals
    dof = 3.0
    x1 = sd.quantiles([distrs[1]], [np.array([0.2, 0.5, 0.999])])[0]
    given = {1: x1}
    w, _, info, l_oo = sd.conditional_factor(jc.CORR3, [1], return_observed=True)
    y_obs = sd.t_scores(sd.normal_scores([distrs[1]], x1[None, :]), dof)
    mu, r = (w @ y_obs).T, sd._conditional_t_scale(y_obs, l_oo, dof)
    probs = np.array([0.0, 0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 1.0, np.nan, -0.1, 1.1])
    q = sd.conditional_quantiles(distrs, probs, given, jc.CORR3, dof=dof)
    assert q.shape == (3, 2, probs.size)
    mapped = sd._t_conditional_quantile_map(probs[None, None, :], mu[:, :, None], r[:, None, None] * info.s[None, :, None], dof, dof + 1.0)
    free = [distrs[0], distrs[2]]
    want = sd.quantiles(free, [mapped[:, m].ravel() for m in range(2)])
    for m in range(2):
        assert _same(q[:, m].ravel(), want[m]), m
        assert np.all(q[:, m, 0] == free[m].domain[0]) and np.all(q[:, m, 8] == free[m].domain[1]) and np.all(np.isnan(q[:, m, 9:]))
        assert np.all(np.diff(q[:, m, :9], axis=1) > 0)
    qs = sd.conditional_quantiles(distrs, probs, {1: float(x1[1])}, jc.CORR3, dof=dof)
    assert qs.shape == (2, probs.size) and _same(qs, q[1])
    inner = slice(1, 8)
    back = sd.conditional_cdfs(distrs, q[:, :, inner], given, jc.CORR3, dof=dof)
    err = np.max(np.abs(back - probs[inner][None, None, :]))
    tol = min(4.0 * ct.MAP_ABS_OBSERVED, ct.MAP_ABS_CAP)
    print(f"\nconditional_cdfs(conditional_quantiles(p, dof), dof) - p: worst {err:.4g} (tolerance {tol:g})")
    assert back.shape == (3, 2, 7) and err <= tol
    for none in (None, np.inf):
        assert _same(sd.conditional_quantiles(distrs, probs, given, jc.CORR3, dof=none), sd.conditional_quantiles(distrs, probs, given, jc.CORR3))
        assert _same(sd.conditional_cdfs(distrs, q[:, :, inner], given, jc.CORR3, dof=none), sd.conditional_cdfs(distrs, q[:, :, inner], given, jc.CORR3))
    # the far set's band is the wider one
    assert np.all(q[2, :, 6] - q[2, :, 2] > 0) and r[2] > 2.0 * r[1]


def test_estimate_methods(hip):
    """Estimate.sample_conditional(dof=3, corr="quadrant") and estimate_conditional_quantiles(dof=3) on the storage of
    tests/test_gpu_t_copula_api.py: what conditional_samples / conditional_quantiles give at the quadrant correlation"""
    from mlmc_amd.tool import simple_distribution as sd
    from tests import concordance_cases as kc
    from tests.test_gpu_concordance_api import _uniform_three
    from tests.test_gpu_normal_scores import _densities, _estimate
    est, dens = _estimate(kc.copula_levels("t")), _densities(_uniform_three())
    distrs = [d[0] for d in dens]
    given = {0: np.array([0.5, 0.999])}
    draws, ok, info = est.sample_conditional(500, SEED, given, corr="quadrant", densities=dens, dof=3)
    corr = est.estimate_quadrant_correlation(densities=dens).corr
    assert draws.shape == (2, 3, 500) and np.all(ok) and info.unobserved.tolist() == [1, 2]
    assert np.all(draws[0, 0] == 0.5) and np.all(draws[1, 0] == 0.999) and np.all((draws[:, 1:] > 0) & (draws[:, 1:] < 1))
    assert _same(draws, sd.conditional_samples(distrs, 500, SEED, given, corr=corr, dof=3))
    gauss, _, _ = est.sample_conditional(500, SEED, given, corr="quadrant", densities=dens)
    assert not _same(gauss, draws) and _same(gauss, est.sample_conditional(500, SEED, given, corr="quadrant", densities=dens, dof=np.inf)[0])
    probs = np.array([0.05, 0.5, 0.95])
    q, ok2 = est.estimate_conditional_quantiles(probs, given, corr="quadrant", densities=dens, dof=3)
    assert q.shape == (2, 2, 3) and np.all(ok2) and np.all(np.diff(q, axis=2) > 0)
    assert _same(q, sd.conditional_quantiles(distrs, probs, given, corr, dof=3))
    qg, _ = est.estimate_conditional_quantiles(probs, given, corr="quadrant", densities=dens)
    # uniform marginals: x is its own uniform.  The far set's band is wider in t scores under the t copula alone
    band = lambda v, nu: np.diff(special.stdtrit(nu, v[..., [0, 2]]), axis=-1)[..., 0]        # noqa: E731
    assert np.all(band(q[1], 3.0) > 2.0 * band(q[0], 3.0))
    zg = special.ndtri(qg[..., [0, 2]])
    assert np.max(np.abs((zg[1, :, 1] - zg[1, :, 0]) - (zg[0, :, 1] - zg[0, :, 0]))) < 1e-6


# ---- errors, no-ops, degenerate problems ---------------------------------------------------------------------------------------------

def test_degenerate_problem(hip, group6):
    """NaN multipliers in one problem among valid ones: its row is NaN in every set, its u_out, z_out and s_out are still written,
    the other rows are bit-equal to a call without it; no error"""
    group = _cycle(group6, 5)
    bad = dict(group[2])
    bad["lam"] = np.full_like(group[2]["lam"], np.nan)
    rng = np.random.default_rng(2)
    F = _scaled_factor(rng, 5, 5)
    shift, scale = rng.uniform(-3.0, 3.0, (2, 5)), np.array([0.5, 2.0])
    want = _tok(hip, group, F, 257, 3.0, 4.0, B=2, shift=shift, scale=scale, want_mass=True)
    for kind in (hip.HOST, hip.DEVICE):
        out, u, z, s, mass = _tok(hip, group[:2] + [bad] + group[3:], F, 257, 3.0, 4.0, B=2, shift=shift, scale=scale, kind=kind,
                                  want_mass=True)
        keep = [0, 1, 3, 4]
        assert np.all(np.isnan(out[:, 2])) and _same(out[:, keep], want[0][:, keep])
        assert _same(u, want[1]) and _same(z, want[2]) and _same(s, want[3]) and np.array_equal(mass[keep], want[4][keep])


def test_errors_and_no_ops(hip, group6):
    group = _cycle(group6, 4)
    rng = np.random.default_rng(4)
    F = jc.random_factor(rng, 4, 3)
    shift = rng.uniform(-1.0, 1.0, (2, 4))

    def expect(rc, pattern):
        with pytest.raises(hip.MlmcHipError, match=pattern):
            hip.check(rc)
    assert _tcond(hip, group, F, 2, 3.0, 5.0, B=2, shift=shift, scale=[0.5, 2.0])[0] == 0
    for bad in (0.999, 64.001, np.nan):
        expect(_tcond(hip, group, F, 2, bad, 5.0)[0], NAME + r": dof must lie in \[1, 64\]")
    for bad in (0.999, 192.001, np.nan):
        expect(_tcond(hip, group, F, 2, 3.0, bad)[0], NAME + r": dof_mix must lie in \[1, 192\]")
    assert _tcond(hip, group, F, 2, 1.0, 1.0)[0] == 0 and _tcond(hip, group, F, 2, 64.0, 192.0)[0] == 0
    assert _tcond(hip, group, F, 2, 64.0, 1.0)[0] == 0                    # dof_mix need not be dof + an integer
    for value in (0.0, -1.0, np.inf, np.nan):
        expect(_tcond(hip, group, F, 2, 3.0, 5.0, B=2, shift=shift, scale=[1.0, value])[0], NAME + ": scale of set 1 ")
    for value in (np.nan, np.inf):
        bad = shift.copy()
        bad[1, 2] = value
        expect(_tcond(hip, group, F, 2, 3.0, 5.0, B=2, shift=bad)[0], NAME + ": shift of set 1, row 2")
    expect(_tcond(hip, group, F, 2, 3.0, 5.0, mix_stream=1)[0], NAME + ": mix_stream equals the stream of latent normal 1")
    expect(_tcond(hip, group, F, 2, 3.0, 5.0, streams=[4, 9, 6], mix_stream=9)[0], NAME + ": mix_stream equals the stream of latent normal 1")
    expect(_tcond(hip, group, F, 2, 3.0, 5.0, B=0)[0], NAME + ": B < 1")
    expect(_tcond(hip, group, F, 2, 3.0, 5.0, B=-3)[0], NAME + ": B < 1")
    for rows in ([0, 1, 1, 2], [0, 2, 1, 3], [-1, 0, 1, 2], [0, 1, 2, 6]):
        expect(_tcond(hip, group, F, 2, 3.0, 5.0, rows=rows, ld_rows=6)[0], NAME + ": rows must be strictly increasing")
    expect(_tcond(hip, group, F, 2, 3.0, 5.0, ld_rows=3)[0], NAME + ": ld_rows < M")
    expect(_tcond(hip, group, F, -1, 3.0, 5.0)[0], NAME + ": n < 0")
    expect(_tcond(hip, group, F, 2, 3.0, 5.0, first=-1)[0], NAME + ": first < 0")
    expect(_tcond(hip, group, F, 2, 3.0, 5.0, kind=5)[0], NAME + ": bad mem_kind")
    expect(_tcond(hip, group, F, 2, 3.0, 5.0, flags=2)[0], NAME + ": unknown flag")
    expect(_tcond(hip, group, F, 2, 3.0, 5.0, flags=ANTITHETIC | SOBOL)[0], NAME)
    expect(_tcond(hip, group, F, 2, 3.0, 5.0, flags=SOBOL, mix_stream=1024)[0], NAME)
    bad = F.copy()
    bad[2] *= np.sqrt(1.0 + 1e-5)
    expect(_tcond(hip, group, bad, 2, 3.0, 5.0)[0], NAME + ": factor row 2.*sum of squares")
    # the elementwise entry: its own range, the other errors of its sibling
    x, out = np.array([0.25, 0.5]), np.full(2, SENTINEL)
    fn = hip.lib().mlmc_chi2_conditional_scale
    for bad in (0.999, 192.001, np.nan, np.inf):
        assert fn(bad, 2, hip.ptr(x), hip.ptr(out), hip.HOST) != 0 and "dof_mix must lie in [1, 192]" in _last_error(hip)
    assert fn(3.0, -1, hip.ptr(x), hip.ptr(out), hip.HOST) != 0 and "n < 0" in _last_error(hip)
    assert fn(3.0, 2, None, hip.ptr(out), hip.HOST) != 0 and "null argument" in _last_error(hip)
    assert fn(3.0, 0, hip.ptr(x), hip.ptr(out), hip.HOST) == 0 and np.all(out == SENTINEL)
    assert fn(1.0, 2, hip.ptr(x), hip.ptr(out), hip.HOST) == 0 and fn(192.0, 2, hip.ptr(x), hip.ptr(out), hip.HOST) == 0
    # no-ops: M = 0, and n = 0 (the arrays may be NULL then and are not touched; the masses are still returned)
    lib, P = hip.lib(), hip.ptr
    assert lib.mlmc_density_sample_conditional_t_batch(0, None, None, None, None, None, None, 0, 0, 0, None, 3.0, 5.0, 1, None, 0, 0, 5, 0, 1,
                                                       None, None, None, 0, None, None, None, None, None, hip.HOST) == 0
    handles, r1, lam, sig = _raw_args(hip, group[:1])
    a = np.array([group[0]["case"].domain[0]])
    b = np.array([group[0]["case"].domain[1]])
    quad = group[0]["quad"]
    one, arr = np.array([[1.0]]), np.full((1, 2), SENTINEL)

    def raw(n=2, out=arr, mass=None):
        return lib.mlmc_density_sample_conditional_t_batch(1, C.cast(handles, C.c_void_p), P(r1), P(lam), P(sig), P(a), P(b), quad[0], quad[1],
                                                           1, P(one), 3.0, 4.0, 1, None, 1, 0, n, 0, 1, None, None, None, 1, P(out), None,
                                                           None, None, P(mass), hip.HOST)
    assert raw() == 0 and np.all(arr != SENTINEL)
    expect(raw(out=None), NAME + ".*null")
    arr[:] = SENTINEL
    assert raw(n=0) == 0 and raw(n=0, out=None) == 0 and np.all(arr == SENTINEL)
    mass = np.full(1, -1.0)
    assert raw(n=0, out=None, mass=mass) == 0
    assert np.array_equal(mass, _quantiles_c(hip, group[:1], quad, np.zeros(0), [0])[1]) and mass[0] > 0
