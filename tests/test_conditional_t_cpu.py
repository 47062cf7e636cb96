"""CPU tests of the conditional entries under the Student-t copula: the fp64 twin of the mixing scale and the t CDF beyond nu = 64,
conditional_factor(return_observed=True), the conditional scale r, the two host maps against the conditional CDF by its definition
(mpmath), and the argument errors that come before any device call."""
import numpy as np
import pytest

from mlmc_amd.tool import simple_distribution as sd
from tests import conditional_cases as cc
from tests import conditional_t_cases as ct
from tests import joint_sample_cases as jc
from tests import t_copula_cases as tc
from tests.test_t_box_cpu import _NoWalk

U = jc.U
NAME = "mlmc_density_sample_conditional_t_batch"


@pytest.mark.parametrize("dof", ct.WIDE_DOFS)
def test_twin_beyond_64(dof):
    """no capped loop of copula_t.hip reaches its cap up to nu = 192, every trip count stays within half its cap, and the mixing
    scale keeps its accuracy: the largest s_units per nu is the recorded one"""
    C, trips = tc.Constants(dof), tc.Trips()
    p = tc.p_arguments()
    s = np.array([tc.twin_chi2_scale(C, float(v), trips) for v in p])
    for y in tc.t_arguments(dof):
        u = tc.twin_t_cdf(C, float(y), trips)
        assert 0.0 <= u <= 1.0
    assert trips.capped == 0
    counts = dict(t_series=(trips.t_series, tc.T_SERIES_CAP), t_lentz=(trips.t_lentz, tc.T_LENTZ_CAP),
                  c_series=(trips.c_series, tc.C_SERIES_CAP), c_lentz=(trips.c_lentz, tc.C_LENTZ_CAP),
                  c_newton=(trips.c_newton, tc.C_NEWTON_CAP))
    assert np.all(np.isfinite(s) & (s > 0.0))
    units = tc.s_units(dof, p, s)
    k = int(np.argmax(units))
    print(f"\nnu {dof:g}: trips " + ", ".join(f"{name} {v[0]}/{v[1]}" for name, v in counts.items())
          + f"; chi2 scale worst {units[k]:.4g} units at p = {p[k]!r} (recorded {ct.S_UNITS_OBSERVED_TWIN_WIDE[dof]})")
    for name, (got, cap) in counts.items():
        assert 2 * got <= cap, (name, got, cap)
    assert units[k] <= jc.tolerance(max(ct.S_UNITS_OBSERVED_TWIN_WIDE.values()))


@pytest.mark.parametrize("observed", [(0,), (2,), (1, 2), (2, 0), ()])
def test_conditional_factor_returns_the_observed_block(observed):
    """L_OO L_OO^T = C'[O, O]; W = L_UO L_OO^-1 is the long-double Schur regression; the default call is unchanged"""
    w, fc, info, l_oo = sd.conditional_factor(jc.CORR3, list(observed), return_observed=True)
    three = sd.conditional_factor(jc.CORR3, list(observed))
    assert len(three) == 3 and np.array_equal(three[0], w) and np.array_equal(three[1], fc) and three[2]._fields == info._fields
    assert all(np.array_equal(a, b) for a, b in zip(three[2], info))
    p = len(observed)
    assert l_oo.shape == (p, p) and l_oo.dtype == np.float64 and np.array_equal(l_oo, np.tril(l_oo))
    used = cc.used_correlation(sd.correlation_factor(jc.CORR3)[0])
    obs = sorted(observed)
    if p:
        assert np.all(np.diag(l_oo) > 0)
        err = np.max(np.abs(l_oo.astype(cc.LD) @ l_oo.T.astype(cc.LD) - used[np.ix_(obs, obs)]))
        want_w, _, _ = cc.schur(used, obs)
        want_l, _, _ = ct.ld_observed(used, obs, np.zeros((p, 1)), 3.0)
        assert err <= 1e-14 and np.max(np.abs(w - want_w)) <= 1e-12 and np.max(np.abs(l_oo - want_l)) <= 1e-14


def test_conditional_scale():
    """r = sqrt((nu + d) / (nu + p)): sqrt(nu / (nu + p)) at d = 0, growing with |y_O|, the long-double value within 4 ulps"""
    used = cc.used_correlation(sd.correlation_factor(jc.CORR3)[0])
    for observed in ((0,), (1, 2), (0, 1)):
        p = len(observed)
        l_oo = sd.conditional_factor(jc.CORR3, list(observed), return_observed=True)[3]
        direction = np.array([1.0, -0.7][:p])
        sizes = np.array([0.0, 0.5, 1.0, 3.0, 6.0, 40.0, 1e6])
        y = direction[:, None] * sizes[None, :]
        for dof in (1.0, 3.0, 30.0, 64.0):
            r = sd._conditional_t_scale(y, l_oo, dof)
            assert r.shape == (sizes.size,) and r[0] == np.sqrt(dof / (dof + p)) and np.all(np.diff(r) > 0)
            _, d, want = ct.ld_observed(used, observed, y, dof)
            assert np.all(np.abs(r - want) <= 4 * U * want.astype(np.float64)), (observed, dof)
            assert d[0] == 0 and np.all(np.diff(d.astype(np.float64)) > 0)
    assert np.array_equal(sd._conditional_t_scale(np.zeros((0, 3)), np.zeros((0, 0)), 3.0), np.ones(3))


def test_host_maps_against_the_definition():
    """p -> p' = T_nu(mu + r s T_{nu + p}^-1(p)) and its inverse, with mu, r and s from conditional_factor and
    _conditional_t_scale, against the conditional CDF of the free t score by its DEFINITION (the ratio of an integral of the
    multivariate t density to the marginal density, mpmath.quad at 30 digits) at the exact t score of p': the absolute errors of
    the CDF map and of the quantile map's inverse, the largest of which is the recorded one"""
    probs = cc.MAP_P
    worst, where = {"cdf map": 0.0, "quantile map": 0.0}, {}
    for dof in ct.MAP_DOFS:
        for corr, observed, y_obs in ct.map_cases():
            p = len(observed)
            w, _, info, l_oo = sd.conditional_factor(corr, list(observed), return_observed=True)
            y_col = np.array(y_obs)[:, None]
            mu = float((w @ y_col)[0, 0])
            scale = float(sd._conditional_t_scale(y_col, l_oo, dof)[0] * info.s[0])
            mapped = sd._t_conditional_quantile_map(probs, mu, scale, dof, dof + p)
            # a mapped probability may round to 1 in fp64 (nu = 30, a given score of 6, p = 1 - 1e-12): its t score is +inf and the
            # reference 1, so the loss shows as an error of the quantile map's inverse
            assert np.all((mapped > 0.0) & (mapped <= 1.0))
            y_exact = ct.mp_t_quantile(dof, mapped, sd._t_quantile_lower_tail(mapped, dof))
            ref = ct.mp_conditional_cdf(corr, y_obs, dof, y_exact)
            assert abs(ref[-1] - 1) <= 1e-20, (dof, y_obs, float(ref[-1] - 1))          # the reference's own error
            ref = np.array([float(v) for v in ref[:-1]])
            back = sd._t_conditional_cdf_map(mapped, mu, scale, dof, dof + p)
            for name, err in (("cdf map", np.abs(back - ref)), ("quantile map", np.abs(ref - probs))):
                k = int(np.argmax(err))
                if err[k] > worst[name]:
                    worst[name], where[name] = float(err[k]), (dof, float(corr[0, 1]), y_obs, float(probs[k]))
    for name, recorded in (("cdf map", ct.MAP_ABS_OBSERVED), ("quantile map", ct.MAP_INVERSE_ABS_OBSERVED)):
        tol = min(4.0 * recorded, ct.MAP_ABS_CAP)
        print(f"\n{name} against the definition: worst absolute error {worst[name]:.4g} at (nu, rho, y_O, p) = {where[name]} "
              f"(recorded {recorded:g}, tolerance {tol:g})")
        assert worst[name] <= tol


def test_host_maps_end_points():
    """p = 0 and 1 map to 0 and 1, what is no probability to NaN; the Gaussian limit: at nu = 64 and a given value at the median
    the mapped probability is within 2e-2 of the Gaussian map"""
    from scipy.special import ndtr, ndtri
    got = sd._t_conditional_quantile_map(np.array([0.0, 1.0, np.nan, -0.1, 1.1]), 0.3, 0.8, 3.0, 4.0)
    assert got[0] == 0.0 and got[1] == 1.0 and np.all(np.isnan(got[2:]))
    p = np.linspace(0.05, 0.95, 19)
    t = sd._t_conditional_quantile_map(p, 0.0, 0.6 * np.sqrt(64.0 / 65.0), 64.0, 65.0)
    assert np.max(np.abs(t - ndtr(0.6 * ndtri(p)))) < 2e-2


def test_argument_errors_before_any_device_call():
    three = [object()] * 3
    given = {0: 1.0}
    for bad in (0.999, 64.001, np.nan, True, "a"):
        with pytest.raises(ValueError, match="dof must lie in"):
            sd.conditional_samples(three, 10, 1, given, corr=jc.CORR3, dof=bad)
        for fn in (sd.conditional_quantiles, sd.conditional_cdfs):
            with pytest.raises(ValueError, match="dof must lie in"):
                fn(three, [0.5], given, jc.CORR3, dof=bad)
    # nu + p beyond 192: 64 + 129 given components of 200
    many, wide = [object()] * 200, {i: 0.0 for i in range(129)}
    with pytest.raises(ValueError, match="exceeds 192"):
        sd.conditional_samples(many, 10, 1, wide, corr=np.eye(200), dof=64.0)
    for fn in (sd.conditional_quantiles, sd.conditional_cdfs):
        with pytest.raises(ValueError, match="exceeds 192"):
            fn(many, [0.5], wide, np.eye(200), dof=64.0)
    with pytest.raises(ValueError, match="mix_stream needs dof"):
        sd.conditional_samples(three, 10, 1, given, corr=jc.CORR3, mix_stream=5)
    with pytest.raises(ValueError, match="return_mixing needs dof"):
        sd.conditional_samples(three, 10, 1, given, corr=jc.CORR3, return_mixing=True)
    with pytest.raises(ValueError, match="return_mixing needs dof"):
        sd.conditional_samples(three, 10, 1, given, corr=jc.CORR3, dof=np.inf, return_mixing=True)
    with pytest.raises(ValueError, match="mix_stream 1 is the stream of a latent normal"):
        sd.conditional_samples(three, 10, 1, given, corr=jc.CORR3, dof=3, mix_stream=1)
    with pytest.raises(ValueError, match="mix_stream 7 is the stream of a latent normal"):
        sd.conditional_samples(three, 10, 1, given, corr=jc.CORR3, dof=3, streams=[4, 7], mix_stream=7)
    with pytest.raises(ValueError, match="mix_stream must be given too"):
        sd.conditional_samples(three, 10, 1, given, corr=jc.CORR3, dof=3, streams=[4, 7])
    with pytest.raises(ValueError, match="below 1024"):
        sd.conditional_samples(three, 10, 1, given, corr=jc.CORR3, dof=3, qmc=True, mix_stream=1024)
    with pytest.raises(ValueError, match="return_observed=True"):
        sd.conditional_samples(three, 10, 1, given, factor_info=sd.conditional_factor(jc.CORR3, [0]), dof=3)
    with pytest.raises(ValueError, match="exactly one of corr"):
        sd.conditional_samples(three, 10, 1, given, dof=3)
    with pytest.raises(ValueError, match="dof_mix must lie in"):
        sd.conditional_mixing_scale(np.array([0.5]), 192.5)
    with pytest.raises(ValueError, match="dof_mix must lie in"):
        sd.conditional_mixing_scale(np.array([0.5]), np.nan)


def test_estimate_argument_errors():
    est = _NoWalk()
    wide = {i: 0.0 for i in range(129)}
    for call in (lambda **kw: est.sample_conditional(4, 1, corr=np.eye(200), **kw),
                 lambda **kw: est.estimate_conditional_quantiles([0.5], corr=np.eye(200), **kw)):
        for bad in (0.5, 100.0, np.nan):
            with pytest.raises(ValueError, match="dof must lie in"):
                call(given={0: 0.1}, dof=bad)
        with pytest.raises(ValueError, match="exceeds 192"):
            call(given=wide, dof=64.0)


def test_entries_are_declared():
    import os
    from mlmc_amd import _lib
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "include", "mlmc_hip.h")).read()
    head = text.split("#define MLMC_ABI_VERSION")[1].split("*/")[0]
    assert NAME in head and "mlmc_chi2_conditional_scale" in head and _lib.ABI_VERSION == 8
    assert len(_lib.SIGNATURES[NAME][1]) == 30 and len(_lib.SIGNATURES["mlmc_chi2_conditional_scale"][1]) == 5
    assert hasattr(_lib.load(), NAME) and hasattr(_lib.load(), "mlmc_chi2_conditional_scale")
