"""CPU tests of the expectations under the max-entropy densities: the calibration of the fp64 twin of tests/density_moment_cases.py
against its long-double reference, the host formulas of simple_distribution.summaries against closed forms, and the argument
checks that raise before any device call."""
import numpy as np
import pytest

from tests import density_moment_cases as mm
from tests import maxent_cases as mc
from tests import maxent_exact as mx

LD = np.longdouble


def test_twin_calibration():
    """the recorded table is what the twin gives: no entry above its record, and every record within 10 % (the second digit of a
    worst case moves with the libm) or one unit of the measurement"""
    worst = mm.twin_table()
    print()
    for key, (v, where) in sorted(worst.items()):
        print(f"twin {key[0]:8s} {key[1]:9s} {key[2]:8s} {v:10.4g} units at {where}")
    for cls in ("regular", "shifted"):
        for col in ("moments", "mass", "entropy"):
            rec = {kind: mm.TWIN_UNITS_M[(cls, kind)][col] for kind in ("converged", "perturbed")}
            got = {kind: worst[(cls, kind, col)][0] for kind in ("converged", "perturbed")}
            if cls == "shifted":                                    # one record for both kinds of multipliers
                got = {kind: max(got.values()) for kind in got}
            for kind in got:
                assert got[kind] <= rec[kind], (cls, kind, col, got[kind])
                assert got[kind] >= min(0.9 * rec[kind], rec[kind] - 1.0), (cls, kind, col, got[kind])


def test_reference_of_a_uniform_density():
    """the sums of the reference at the constant density rho = exp(-lambda_0), lambda_0 = fl(log W): Legendre moments T e_0, mass
    T = W rho, entropy column T lambda_0, to long-double rounding (the moments to the fp64 rounding of the
    transform constants scale = 2 / W and shift, which are data of the test basis)"""
    dom = (-4.0, 6.0)
    case = mc.Case("uniform", mx.Desc(mx.LEGENDRE, 2, dom), np.eye(2)[0], np.ones(2), np.array([np.log(10.0), 0.0]), "other")
    for quad in mm.RULES:
        K = min(8, 2 * quad[1])                                     # a rule of n nodes per cell is exact up to degree 2 n - 1
        vals, scale = mm.moment_sums(case, case.lam0, mx.Desc(mx.LEGENDRE, 8, dom), K, quad)
        T = 10 * np.exp(-LD(case.lam0[0]))
        assert np.all(np.abs(vals["moments"] - T * np.eye(8)[0, :K]) < 1e-15) and abs(vals["mass"] - T) < 1e-17
        assert abs(vals["entropy"] - T * LD(case.lam0[0])) < 1e-17 and np.all(scale["moments"] > 0.99)


def _t_moments(pdf_moment, ref):
    """normalised E[t^k], k = 0 .. 4, of t on ref = (lo, hi) from an exact k-th raw moment function"""
    return np.array([[float(pdf_moment(k)) for k in range(5)]])


def test_summary_formulas_uniform():
    """exact sums of a uniform density on (a, b), t = (x - m) / W about any centre m: mean (a + b) / 2, variance W^2 / 12, skewness 0,
    kurtosis 9 / 5"""
    from mlmc_amd.tool import simple_distribution as sd
    for a, b, m in ((-4.0, 6.0, 1.0), (-4.0, 6.0, -1.5), (1e3, 1e3 + 1e-2, 1e3 + 4e-3), (0.5, 3.0, 0.5)):
        W = b - a
        lo, hi = LD(a - m) / LD(W), LD(b - m) / LD(W)
        r = np.array([[float((hi ** (k + 1) - lo ** (k + 1)) / (k + 1) / (hi - lo)) for k in range(5)]])
        scale = (float(hi) - float(lo)) / W
        mean, var, skew, kurt = sd._central_summary(r, np.array([scale]), np.array([float(lo)]), np.array([a]))
        assert abs(mean[0] - 0.5 * (a + b)) <= 1e-14 * max(abs(a), abs(b)) and abs(var[0] - W * W / 12) <= 1e-13 * W * W
        assert abs(skew[0]) <= 1e-12 and abs(kurt[0] - 1.8) <= 1e-12


def test_summary_formulas_exponential():
    """exact sums of exp(-x) on (0, 40) (the truncation is below 1e-15): mean 1, variance 1, skewness 2, kurtosis 9, about a
    centre next to the mean (as `summaries` chooses it) and about one far from it"""
    from math import factorial
    from mlmc_amd.tool import simple_distribution as sd
    a, b = 0.0, 40.0
    W = b - a
    for m in (1.0, 1.0 + 1e-9, 3.0):
        # E[(x - m)^k] = sum_j C(k, j) j! (-m)^(k - j)
        c = [sum(LD(factorial(k)) / factorial(k - j) * LD(-m) ** (k - j) for j in range(k + 1)) for k in range(5)]
        r = np.array([[float(c[k] / LD(W) ** k) for k in range(5)]])
        ref0 = (a - m) / W
        mean, var, skew, kurt = sd._central_summary(r, np.array([1.0 / W]), np.array([ref0]), np.array([a]))
        tol = 1e-13 if m < 2 else 1e-11
        assert abs(mean[0] - 1) <= tol and abs(var[0] - 1) <= tol and abs(skew[0] - 2) <= 10 * tol and abs(kurt[0] - 9) <= 100 * tol


def test_entropy_normalisation():
    from mlmc_amd.tool import simple_distribution as sd
    # rho = 2 / W on (0, W): raw column -int rho log rho = -2 log(2 / W), mass 2; the normalised density 1 / W has entropy log W
    W = 5.0
    got = sd._normalized_entropy(np.array([-2 * np.log(2 / W)]), np.array([2.0]))
    assert abs(got[0] - np.log(W)) < 1e-15


def test_names_exist():
    import mlmc_amd._lib as _lib
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.tool import distribution, simple_distribution as sd
    assert "mlmc_density_moments_batch" in _lib.SIGNATURES and len(_lib.SIGNATURES["mlmc_density_moments_batch"][1]) == 14
    assert sd.DensityMoments._fields == ("moments", "entropy", "mass")
    assert sd.DensitySummary._fields == ("mean", "var", "skewness", "kurtosis", "entropy", "mass")
    for name in ("density_moments", "summaries"):
        assert callable(getattr(sd, name))
    for cls in (sd.SimpleDistribution, distribution.Distribution):
        for name in ("fitted_moments", "summary", "entropy"):
            assert callable(getattr(cls, name))
    for name in ("estimate_component_summaries", "bootstrap_component_summaries"):
        assert callable(getattr(Estimate, name))
    header = open(__import__("os").path.join(__import__("os").path.dirname(__file__), "..", "include", "mlmc_hip.h")).read()
    assert "int mlmc_density_moments_batch(" in header


class _NoDevice:
    """a moments object whose device handle must not be asked for"""

    def __init__(self, fn):
        self.__class__ = type("NoDevice" + type(fn).__name__, (type(fn),), {"_basis_handle": _NoDevice._refuse})
        self.__dict__.update(fn.__dict__)

    @staticmethod
    def _refuse(self):
        raise AssertionError("a device call was made")


def _dists(n, quad=(64, 21)):
    import mlmc_amd
    from mlmc_amd.tool import simple_distribution as sd
    out = []
    for i in range(n):
        dom = (-1.0 - i, 2.0)
        d = sd.SimpleDistribution(_NoDevice(mlmc_amd.Legendre(4, dom)), np.stack([np.eye(4)[0], np.ones(4)], axis=1), domain=dom)
        d.multipliers, d._moment_errs = np.array([1.0, 0.0, 0.0, 0.0]), np.ones(4)
        d.n_intervals, d._gauss_degree = quad
        out.append(d)
    return out


def test_argument_checks_raise_before_any_device_call():
    import mlmc_amd
    from mlmc_amd.tool import simple_distribution as sd
    d = _dists(3)
    fns = [_NoDevice(mlmc_amd.Legendre(6, x.domain)) for x in d]
    with pytest.raises(ValueError, match="density_moments: 2 moments objects for 3 distributions"):
        sd.density_moments(d, fns[:2])
    with pytest.raises(ValueError, match="density_moments: 2 sizes for 3 distributions"):
        sd.density_moments(d, fns, [3, 3])
    for bad in (0, 7, -1, 2.0, True):
        with pytest.raises(ValueError, match="density_moments: distribution 1: size must be an integer in 1..6"):
            sd.density_moments(d, fns, [3, bad, 3])
    with pytest.raises(ValueError, match="density_moments: distribution 0: size must be an integer in 1..4"):
        sd.density_moments(d, None, 5)
    with pytest.raises(ValueError, match="density_moments: moments_fns must hold Moments objects"):
        sd.density_moments(d, [fns[0], "legendre", fns[2]])
    other = _dists(1, quad=(32, 21))
    with pytest.raises(ValueError, match="density_moments: every distribution must use the same quadrature"):
        sd.density_moments(d + other, fns + [fns[0]])
    with pytest.raises(ValueError, match="summaries: every distribution must use the same quadrature"):
        sd.summaries(d + other)
    with pytest.raises(ValueError, match="density_moments: 1 moments objects for 0 distributions"):
        sd.density_moments([], [fns[0]])
    empty = sd.density_moments([])
    assert empty.moments == [] and empty.entropy.shape == (0,) and empty.mass.shape == (0,)
    assert all(v.shape == (0,) for v in sd.summaries([]))
