"""CPU tests of the tail means (expected shortfall): the calibration of the fp64 twin against the long-double reference
(tests/tail_cases.py), the reference against its own definition, and the boundary of the new entry (declared, bound, exported,
ABI version unchanged; no CPU fallback of the Python entries)."""
import os
import re

import numpy as np
import pytest

from tests import maxent_cases as mc
from tests import quantile_cases as qc
from tests import tail_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "mlmc_density_tail_means_batch"
LD = np.longdouble

_PROBLEMS = None


def _problems():
    """the table at fp64 Newton multipliers (the device is not involved)"""
    global _PROBLEMS
    if _PROBLEMS is None:
        _PROBLEMS = qc.problems(lambda case, quad: mc.newton_f64(case, quad))
    return _PROBLEMS


def _mix_r9():
    case = mc.cases()["mix_R9"]
    lam = [l for c, k, l, q, r in _problems() if c.name == "mix_R9" and k == "converged" and q == (64, 21)][0]
    return case, lam


def test_grid():
    assert tc.GRID.size == 54 and np.all(np.diff(tc.GRID) > 0)
    assert set(qc.GRID[::4]) <= set(tc.GRID) and {qc.GRID[0], qc.GRID[1], qc.GRID[-2], qc.GRID[-1]} <= set(tc.GRID)


def test_twin_calibration():
    """The fp64 twin of the tail means against the long-double reference at x = the twin's quantiles, over every used problem
    (exactly qc.used_problems) and the grid: the worst error per tolerance class stays at or below the recorded TWIN_UNITS_T,
    which set the device tolerance."""
    used = qc.used_problems(_problems())
    left = [(c.name, k, q) for c, k, l, q, r in _problems() if r > qc.RESOLVED_RTOL]
    assert len(used) + len(left) == len(_problems()) and all(k == "perturbed" and n in qc.MAY_BE_UNRESOLVED for n, k, q in left)
    worst = {}
    for case, kind, lam, quad in used:
        x = qc.twin_quantiles(case, lam, quad, tc.GRID)
        lower, upper, _, _ = tc.TailTable(case, lam, quad, np.float64).tails(x)
        ul, uu = tc.tail_units(tc.TailTable(case, lam, quad), x, lower, upper)
        cls = mc.tolerance_class(case)
        for name, u in (("lower", ul), ("upper", uu)):
            k = int(np.argmax(u))
            if u[k] > worst.get(cls, (-1.0, None))[0]:
                worst[cls] = (float(u[k]), f"{case.name} {kind} {quad[0]}x{quad[1]} {name} p = {tc.GRID[k]:.6g}")
    print()
    for cls, (v, where) in sorted(worst.items()):
        print(f"twin tail means: worst {cls:8s} {v:10.4g} units at {where} (recorded {tc.TWIN_UNITS_T[cls]:g})")
    print("left out:", left)
    assert set(worst) == set(tc.TWIN_UNITS_T)
    for cls, (v, where) in worst.items():
        assert v <= tc.TWIN_UNITS_T[cls], (cls, v, where)
    assert tc.tail_tolerance(mc.cases()["mix_R9"]) == max(16.0, 4.0 * tc.TWIN_UNITS_T["regular"])
    assert tc.tail_tolerance(mc.cases()["shifted_R6"]) == max(16.0, 4.0 * tc.TWIN_UNITS_T["shifted"])


def test_reference_is_the_definition():
    case, lam = _mix_r9()
    ref = tc.TailTable(case, lam, (64, 21))
    a, b = case.domain
    quantile_table = qc.RuleTable(case, lam, (64, 21))
    assert np.array_equal(ref.P, quantile_table.P) and ref.T == quantile_table.T            # the table of the quantile checks
    assert ref.S[-1] == 0 and ref.W[-1] == 0 and ref.V[0] == 0 and ref.P[0] == 0
    assert abs(ref.S[0] - ref.T) <= 1e-18 * ref.T
    mean, _ = ref.mean()
    lower, upper, sl, su = ref.tails([a, b])
    assert lower[0] == a and upper[1] == b                                                  # tails without mass
    assert abs(lower[1] - mean) <= 4 * np.finfo(LD).eps * (abs(a) + abs(b))                 # lower(b) = mean, in long double
    assert abs(upper[0] - mean) <= qc.RESOLVED_RTOL * (b - a)                               # upper(a): up to the rule's resolution
    # a + V / T and b - W / T are the same mean (up to the long-double rounding of sums of 1344 terms)
    assert abs((ref.b - ref.W[0] / ref.S[0]) - mean) <= 1e-16 * (b - a)
    x = np.linspace(a, b, 1001)
    lower, upper, sl, su = ref.tails(x)
    assert np.all(lower <= x) and np.all(x <= upper)
    assert np.all(np.diff(lower) >= 0) and np.all(np.diff(upper) >= 0)
    assert np.all(sl >= np.abs(lower)) and np.all(su >= np.abs(upper))
    lower, upper, _, _ = ref.tails([np.nan, 0.5])
    assert np.isnan(lower[0]) and np.isnan(upper[0]) and np.isfinite(lower[1]) and np.isfinite(upper[1])
    # at an edge the partial cell [e_j, e_j] is empty: lower(e_j) = a + V_j / P_j
    j = 20
    lower, upper, _, _ = ref.tails([ref.e[j]])
    assert abs(lower[0] - (ref.a + ref.V[j] / ref.P[j])) <= 1e-17 * (b - a)


def test_order_and_ends_on_every_class():
    """lower <= x <= upper and the end-point conventions on a shifted, a log and a transformed problem of the table"""
    for name in ("shifted_R6", "log_legendre_R8", "norm12_R21"):
        case = mc.cases()[name]
        lam = [l for c, k, l, q, r in _problems() if c.name == name and k == "converged" and q == (64, 21)][0]
        ref = tc.TailTable(case, lam, (64, 21))
        a, b = case.domain
        x = np.linspace(a, b, 101)
        x[0], x[-1] = a, b
        lower, upper, _, _ = ref.tails(x)
        assert lower[0] == a and upper[-1] == b, name
        assert np.all(lower <= x) and np.all(x <= upper), name
        assert np.all(np.diff(lower) >= 0) and np.all(np.diff(upper) >= 0), name
        mean, _ = ref.mean()
        assert abs(lower[-1] - mean) <= 4 * np.finfo(LD).eps * (abs(a) + abs(b)), name
        assert abs(upper[0] - mean) <= qc.RESOLVED_RTOL * (b - a), name


def test_entry_is_declared_bound_and_exported():
    from mlmc_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "mlmc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+" + ENTRY + r"\s*\(", code)
    assert ENTRY in _lib.SIGNATURES and hasattr(lib, ENTRY)
    comment = text.split("#define MLMC_ABI_VERSION")[1].split("*/")[0]
    assert ENTRY in comment.split("added within 8")[1], ENTRY + " is not named in the version comment"
    assert len(_lib.SIGNATURES[ENTRY][1]) == 17
    assert _lib.ABI_VERSION == 8 and lib.mlmc_abi_version() == 8
    assert re.search(r"#define\s+MLMC_ABI_VERSION\s+8\b", text)


def test_no_cpu_fallback_of_the_new_entries():
    """without a device the new Python entries raise like every other compute call"""
    import torch
    from mlmc_amd import _lib, Legendre
    from mlmc_amd.tool import simple_distribution as sd
    from mlmc_amd.tool.distribution import Distribution
    q, lower, upper, mean = sd.tail_means([], [0.5])
    assert q == [] and lower == [] and upper == [] and len(mean) == 0
    dom = (-1.0, 1.0)
    data = np.stack([np.eye(4)[0], np.ones(4)], axis=1)
    d = sd.SimpleDistribution(Legendre(4, dom), data, domain=dom)
    d._initialize_params(4, 1e-8)
    old = Distribution(Legendre(4, dom), data.copy(), domain=dom)
    old.multipliers, old._moment_errs = d.multipliers, d.moment_errs
    for dist in (d, old):
        with pytest.raises(ValueError, match="tail must be"):
            dist.expected_shortfall(0.5, tail="both")
    if torch.cuda.is_available():
        return
    for call in (lambda: sd.tail_means([d], [0.5]), lambda: d.expected_shortfall(0.5), lambda: d.expected_shortfall([0.1], "lower"),
                 lambda: old.expected_shortfall([0.5])):
        with pytest.raises(_lib.MlmcHipError):
            call()


def test_estimate_entries_without_a_device():
    """the Estimate methods exist, check `tail` before any device work and raise MlmcHipError without a device"""
    import torch
    from mlmc_amd import _lib, Legendre, estimator
    from mlmc_amd.tool import simple_distribution as sd
    assert callable(estimator.Estimate.estimate_component_shortfall) and callable(estimator.Estimate.bootstrap_component_shortfall)
    est = estimator.Estimate(None, None, None)
    with pytest.raises(ValueError, match="estimate_component_shortfall: tail must be"):
        est.estimate_component_shortfall([0.5], tail="two-sided")
    with pytest.raises(ValueError, match="bootstrap_component_shortfall: tail must be"):
        est.bootstrap_component_shortfall([0.5], 4, tail=None)
    if torch.cuda.is_available():
        return
    dom = (-1.0, 1.0)
    d = sd.SimpleDistribution(Legendre(4, dom), np.stack([np.eye(4)[0], np.ones(4)], axis=1), domain=dom)
    d._initialize_params(4, 1e-8)
    densities = [(d, None, type("R", (), {"success": True})(), None)]
    with pytest.raises(_lib.MlmcHipError):
        est.estimate_component_shortfall([0.05, 0.95], "lower", densities=densities)
