"""CPU tests of the Student-t copula: the host functions (bivariate_t_orthant, fit_copula_dof, the argument checks of every new
Python entry) and the algorithm twin of the device functions against mpmath.  Nothing here touches a device."""
import math

import mpmath
import numpy as np
import pytest
from scipy import special, stats

from mlmc_amd import estimator
from mlmc_amd.tool import simple_distribution as sd
from tests import concordance_cases as cc
from tests import joint_sample_cases as jc
from tests import t_copula_cases as tc

# The reference below is exact to 1e-20 and better (mpmath reports its own error), so the tolerance is the implementation's: its
# rule leaves the two outermost panels of the mixing probability (mass 1e-6 each) to 96 nodes that meet an endpoint singularity
# there; a relative error of 1e-3 on those panels is 1e-9 absolute.  The issue allows no more than 1e-8.
ORTHANT_TOL = 1e-9


def _mp_t_cdf(nu, y):
    low = mpmath.betainc(nu / 2, mpmath.mpf(1) / 2, 0, nu / (nu + y * y), regularized=True) / 2
    return low if y <= 0 else 1 - low


def mp_t_orthant(h, k, rho, dof):
    """P(T1 > h, T2 > k) of the bivariate t density over [h, inf) x [k, inf) at 25 digits: the inner integral in closed form (given
    T1 = t, T2 is rho t + sqrt((nu + t^2) (1 - rho^2) / (nu + 1)) times a t variate with nu + 1 degrees of freedom), the outer one by
    mpmath.quad, which also states its error -> (value, error)"""
    with mpmath.workdps(25):
        nu, rho, h, k = mpmath.mpf(float(dof)), mpmath.mpf(float(rho)), mpmath.mpf(float(h)), mpmath.mpf(float(k))
        c = mpmath.gamma((nu + 1) / 2) / (mpmath.sqrt(nu * mpmath.pi) * mpmath.gamma(nu / 2))

        def f(t):
            scale = mpmath.sqrt((nu + t * t) * (1 - rho * rho) / (nu + 1))
            return c * (1 + t * t / nu) ** (-(nu + 1) / 2) * (1 - _mp_t_cdf(nu + 1, (k - rho * t) / scale))
        value, err = mpmath.quad(f, [h, h + 1, h + 3, h + 10, h + 100, mpmath.inf], error=True)
        return float(value), float(err)


@pytest.fixture(scope="module")
def orthant_reference():
    """the grid of the accuracy test, evaluated once"""
    rows = []
    for dof in (1.0, 3.0, 4.5, 30.0):
        for rho in (0.0, 0.6, -0.5, 0.95):
            for p in (0.5, 0.9, 0.99):
                h = float(stats.t.ppf(p, dof))
                rows.append((dof, rho, p, h) + mp_t_orthant(h, h, rho, dof))
    return rows


def test_orthant_against_the_quadrature_of_the_density(orthant_reference):
    worst = 0.0
    for dof, rho, p, h, ref, err in orthant_reference:
        assert 10.0 * err <= ORTHANT_TOL
        got = sd.bivariate_t_orthant(h, h, rho, dof)
        worst = max(worst, abs(got - ref))
        assert abs(got - ref) <= ORTHANT_TOL, (dof, rho, p, got, ref)
    print("bivariate_t_orthant: largest error against mpmath {:.2e} (tolerance {:.0e})".format(worst, ORTHANT_TOL))


def test_orthant_vectorises_and_takes_the_limits():
    h = np.array([[0.3], [1.5]])
    rho = np.array([-0.5, 0.0, 0.6])
    out = sd.bivariate_t_orthant(h, 0.2, rho, 4.5)
    assert out.shape == (2, 3)
    for i in range(2):
        for j in range(3):
            assert out[i, j] == sd.bivariate_t_orthant(h[i, 0], 0.2, rho[j], 4.5)
    # |rho| = 1: P(T > max(h, k)) and max(0, P(T > k) - P(T < h))
    assert abs(sd.bivariate_t_orthant(0.3, 1.1, 1.0, 3) - stats.t.sf(1.1, 3)) < ORTHANT_TOL
    assert abs(sd.bivariate_t_orthant(-0.3, 0.1, -1.0, 3) - (stats.t.sf(0.1, 3) - stats.t.cdf(-0.3, 3))) < ORTHANT_TOL


def test_orthant_at_infinite_and_large_dof():
    h = special.ndtri(np.array([0.5, 0.9, 0.99]))
    for rho in (0.0, 0.6, -0.5, 0.95):
        normal = sd.bivariate_orthant(h, h, rho)
        assert np.array_equal(sd.bivariate_t_orthant(h, h, rho, np.inf), normal)
        # nu = 64 is not yet the normal law: the difference from it is the true one
        got = sd.bivariate_t_orthant(h, h, rho, 64.0)
        true = np.array([mp_t_orthant(v, v, rho, 64.0)[0] for v in h])
        assert np.max(np.abs((got - normal) - (true - normal))) <= ORTHANT_TOL
        assert np.max(np.abs(true - normal)) > 1e-4


def test_median_identity():
    for dof in (1, 3, 30):
        for rho in (-0.5, 0.0, 0.6, 0.95):
            assert abs(sd.bivariate_t_orthant(0.0, 0.0, rho, dof) - (0.25 + math.asin(rho) / (2.0 * math.pi))) <= 1e-12


def test_zero_correlation_is_not_independence():
    h = float(stats.t.ppf(0.9, 3))
    assert abs(sd.bivariate_t_orthant(h, h, 0.0, 3) - 0.1 ** 2) > 1e-3


# ---- the fit on the twin counts ----------------------------------------------------------------------------------------------

def _twin_statistics(levels, lower, upper):
    counts = [cc.twin_counts(f, c, lower, upper) for f, c in levels]
    n = np.array([c[2] for c in counts])
    _, _, prob, var = cc.twin_level_statistics(n, np.array([c[0] for c in counts]))
    return prob, var


@pytest.fixture(scope="module", params=["t", "gauss"])
def twin_case(request):
    levels = cc.copula_levels(request.param)
    prob, var = _twin_statistics(levels, *cc.upper_events(cc.PROBS, 3))
    half, half_var = _twin_statistics(levels, *cc.upper_events([0.5], 3))
    quadrant, stderr = estimator.quadrant_correlation(half[0], half_var[0])
    return request.param, prob, var, quadrant, stderr


def _check_fit(kind, fit):
    grid = list(fit.grid)
    print(kind, "objective over the grid:", " ".join("{:g}:{:.1f}".format(g, o) for g, o in zip(grid, fit.objective)))
    if kind == "t":
        assert fit.dof == 3.0
        assert fit.objective[grid.index(3.0)] < 6 * 5.0 ** 2
        assert fit.objective[grid.index(2.0)] > 100.0 and fit.objective[grid.index(4.0)] > 100.0
    else:
        assert fit.dof == np.inf
        assert fit.objective[grid.index(3.0)] > 1000.0


def test_fit_finds_the_degrees_of_freedom(twin_case):
    kind, prob, var, _, _ = twin_case
    fit = sd.fit_copula_dof(prob, var, cc.PROBS, cc.CORR)
    assert fit.z.shape == (len(sd.COPULA_DOF_GRID), 2, 3, 3) and fit.objective.shape == (len(sd.COPULA_DOF_GRID),)
    assert np.all(np.isnan(fit.z[:, :, np.arange(3), np.arange(3)]))
    iu = np.triu_indices(3, 1)
    assert np.allclose(fit.objective, np.sum(fit.z[:, :, iu[0], iu[1]] ** 2, axis=(1, 2)), rtol=1e-14)
    _check_fit(kind, fit)


def test_fit_with_the_quadrant_correlation(twin_case):
    kind, prob, var, quadrant, stderr = twin_case
    iu = np.triu_indices(3, 1)
    print(kind, "quadrant correlation", quadrant[iu], "stderr", stderr[iu])
    assert np.all(np.abs(quadrant[iu] - cc.CORR[iu]) <= 5.0 * stderr[iu])
    assert np.all(np.diag(quadrant) == 1.0) and np.all(np.diag(stderr) == 0.0)
    _check_fit(kind, sd.fit_copula_dof(prob, var, cc.PROBS, quadrant))


def test_fit_breaks_a_tie_towards_the_larger_dof():
    prob = np.full((1, 2, 2), 0.3)
    fit = sd.fit_copula_dof(prob, np.full((1, 2, 2), np.nan), [0.5], np.eye(2), grid=(3, 10, np.inf))
    assert np.all(fit.objective == 0.0) and fit.dof == np.inf


# ---- argument checks, before anything touches the device -------------------------------------------------------------------

def test_argument_checks():
    with pytest.raises(ValueError, match="dof must lie in"):
        sd.joint_samples([object()], 4, 1, corr=np.eye(1), dof=0.5)
    with pytest.raises(ValueError, match="dof must lie in"):
        sd.joint_samples([object()], 4, 1, corr=np.eye(1), dof=65.0)
    with pytest.raises(ValueError, match="dof must lie in"):
        sd.joint_samples([object()], 4, 1, corr=np.eye(1), dof=np.nan)
    with pytest.raises(ValueError, match="dof must lie in"):
        sd.joint_samples([object()], 4, 1, corr=np.eye(1), dof=True)
    with pytest.raises(ValueError, match="return_mixing needs dof"):
        sd.joint_samples([object()], 4, 1, corr=np.eye(1), return_mixing=True)
    with pytest.raises(ValueError, match="mix_stream needs dof"):
        sd.joint_samples([object()], 4, 1, corr=np.eye(1), mix_stream=3)
    with pytest.raises(ValueError, match="mix_stream must be given"):
        sd.joint_samples([object()] * 2, 4, 1, corr=np.eye(2), streams=[0, 1], dof=3)
    with pytest.raises(ValueError, match="is the stream of a latent normal"):
        sd.joint_samples([object()] * 2, 4, 1, corr=np.eye(2), streams=[4, 7], dof=3, mix_stream=7)
    with pytest.raises(ValueError, match="is the stream of a latent normal"):
        sd.joint_samples([object()] * 2, 4, 1, corr=np.eye(2), dof=3, mix_stream=1)
    with pytest.raises(ValueError, match="mix_stream must be an integer"):
        sd.joint_samples([object()] * 2, 4, 1, corr=np.eye(2), dof=3, mix_stream=-1)
    with pytest.raises(ValueError, match="dof together with given"):
        sd.joint_aggregates([object()] * 2, 4, 1, corr=np.eye(2), dof=3, given={0: 0.1})
    with pytest.raises(ValueError, match="dof must lie in"):
        sd.joint_aggregates([object()] * 2, 4, 1, corr=np.eye(2), dof=0.0)
    for fn in (sd.student_t_cdf, sd.chi2_mixing_scale):
        for bad in (0.99, 64.5, np.nan, np.inf, None):
            with pytest.raises(ValueError, match="dof must"):
                fn(np.zeros(3), bad)
    with pytest.raises(ValueError, match="dof must be one positive number"):
        sd.bivariate_t_orthant(0.0, 0.0, 0.5, -1.0)
    with pytest.raises(ValueError, match="rho must lie"):
        sd.bivariate_t_orthant(0.0, 0.0, 1.5, 3.0)
    ok = np.full((1, 2, 2), 0.3)
    for grid in ((0.5, 3), (3, 65), (3, np.nan), ()):
        with pytest.raises(ValueError, match="the grid must hold"):
            sd.fit_copula_dof(ok, ok, [0.9], np.eye(2), grid=grid)
    with pytest.raises(ValueError, match="prob and var must be"):
        sd.fit_copula_dof(ok[0], ok[0], [0.9], np.eye(2))
    with pytest.raises(ValueError, match="probability levels"):
        sd.fit_copula_dof(ok, ok, [1.0], np.eye(2))
    with pytest.raises(ValueError, match="corr must be a finite"):
        sd.fit_copula_dof(ok, ok, [0.9], np.eye(3))


class _NoWalk(estimator.Estimate):
    """an Estimate whose quantity must not be touched: the checks under test come first"""

    def __init__(self):
        pass


def test_estimate_argument_checks():
    est = _NoWalk()
    with pytest.raises(ValueError, match="dof must lie in"):
        est.sample_joint(4, 1, corr=np.eye(2), dof=0.5)
    with pytest.raises(ValueError, match="dof must lie in"):
        est.estimate_tail_dependence(corr=np.eye(2), dof=100.0)
    with pytest.raises(ValueError, match="the grid must hold"):
        est.estimate_copula_dof(corr=np.eye(2), grid=(0.5, 3))


# ---- the algorithm twin of the device functions ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def twin_table():
    """per nu: the largest error of the twin in its units on the arguments of this file, and the trips of every capped loop"""
    rows = []
    for dof in tc.DOFS:
        C, trips = tc.Constants(dof), tc.Trips()
        y = tc.t_arguments(dof)
        u = np.array([tc.twin_t_cdf(C, float(v), trips) for v in y])
        t_units = tc.t_units(u, tc.mp_t_cdf(dof, y))
        p = tc.p_arguments()
        s = np.array([tc.twin_chi2_scale(C, float(v), trips) for v in p])
        rows.append(dict(dof=dof, y=y, u=u, t_units=t_units, p=p, s=s, s_units=tc.s_units(dof, p, s), trips=trips))
    return rows


def test_twin_against_mpmath(twin_table):
    print("\n  nu | T units (at y)          | s units (at p)          | trips: t series, t fraction, P series, Q fraction, Newton")
    for r in twin_table:
        i, k, t = int(np.argmax(r["t_units"])), int(np.argmax(r["s_units"])), r["trips"]
        print("{:4g} | {:8.2f} ({:12.5g}) | {:8.2f} ({:12.5g}) | {} {} {} {} {}".format(
            r["dof"], r["t_units"][i], r["y"][i], r["s_units"][k], r["p"][k], t.t_series, t.t_lentz, t.c_series, t.c_lentz, t.c_newton))
    for r in twin_table:
        assert np.max(r["t_units"]) <= jc.tolerance(tc.T_UNITS_OBSERVED_TWIN), r["dof"]
        assert np.max(r["s_units"]) <= jc.tolerance(tc.S_UNITS_OBSERVED_TWIN), r["dof"]


def test_twin_reaches_no_cap(twin_table):
    for r in twin_table:
        t = r["trips"]
        assert t.capped == 0, r["dof"]
        assert t.t_series < tc.T_SERIES_CAP and t.t_lentz < tc.T_LENTZ_CAP and t.c_series < tc.C_SERIES_CAP
        assert t.c_lentz < tc.C_LENTZ_CAP and t.c_newton < tc.C_NEWTON_CAP


def test_twin_properties(twin_table):
    for r in twin_table:
        C, trips = tc.Constants(r["dof"]), tc.Trips()
        assert np.all(np.isfinite(r["s"]) & (r["s"] > 0.0))
        ordered = r["s"][np.argsort(r["p"])]                               # s falls as p grows, up to the rounding where the side switches
        assert np.all(np.diff(ordered) <= 4.0 * 2.0 ** -52 * ordered[1:])
        pos = r["y"] > 0.0
        mirrored = np.array([1.0 - tc.twin_t_cdf(C, -float(v), trips) for v in r["y"][pos]])
        assert np.array_equal(r["u"][pos], mirrored)
        assert tc.twin_t_cdf(C, -math.inf, trips) == 0.0 and tc.twin_t_cdf(C, math.inf, trips) == 1.0
        assert math.isnan(tc.twin_t_cdf(C, math.nan, trips)) and tc.twin_t_cdf(C, 0.0, trips) == 0.5
        for bad in (0.0, 1.0, -0.5, 1.5, math.nan):
            assert math.isnan(tc.twin_chi2_scale(C, bad, trips))


# ---- the host restatement of the draws whose statistics the device test checks --------------------------------------------------

def test_host_restatement_of_the_statistics_case():
    """the draws of the statistics test of tests/test_gpu_t_copula.py restated with SciPy's functions: the bounds that the device
    draws must meet hold for the law itself under this seed"""
    F = np.linalg.cholesky(cc.CORR)
    n = tc.STAT_N
    z = jc.normals(tc.STAT_SEED, [0, 1, 2], 0, n)
    s = np.sqrt(tc.STAT_DOF / stats.chi2.ppf(tc.mixing_uniforms(tc.STAT_SEED, 3, 0, n), tc.STAT_DOF))
    u = tc.clamp(stats.t.cdf((F @ z) * s, tc.STAT_DOF))
    pair, _, kept = cc.twin_counts(u, None, *cc.upper_events(tc.STAT_PROBS, 3))
    res = tc.concordance_z(pair, kept)
    print("host restatement: |z| under the t model", np.round(np.abs(res["z_t"]).max(axis=1), 2), "z under the Gaussian model at 0.9",
          np.round(res["z_gauss"][1], 2))
    assert np.max(np.abs(res["z_t"])) < tc.STAT_Z_BOUND
    assert np.min(res["z_gauss"][1]) > tc.STAT_Z_GAUSS
    assert res["fit"].dof == tc.STAT_DOF
