"""CPU tests of the CDF / quantile checks: the calibration of the fp64 twin against the long-double reference
(tests/quantile_cases.py), the list of unresolved problems computed from the reference alone, and the boundary of the three new
entries (declared, bound, exported; no CPU fallback)."""
import os
import re

import numpy as np
import pytest

from tests import maxent_cases as mc
from tests import quantile_cases as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mlmc_density_integrate_batch", "mlmc_density_cdf_batch", "mlmc_density_quantiles_batch")

_PROBLEMS = None


def _problems():
    """the table at fp64 Newton multipliers (the device is not involved)"""
    global _PROBLEMS
    if _PROBLEMS is None:
        _PROBLEMS = qc.problems(lambda case, quad: mc.newton_f64(case, quad))
    return _PROBLEMS


def test_unresolved_problems_are_the_named_ones():
    """No converged problem and at most the four named perturbed ones are left out, decided on the long-double masses of the
    rule and of the 4 x finer rule; the resolution of every problem is printed (-s)."""
    probs = _problems()
    assert len(probs) == 2 * 2 * len(mc.cases())
    print()
    for case, kind, lam, quad, res in probs:
        print(f"resolution {case.name:26s} {kind:9s} {quad[0]}x{quad[1]}: {res:.3g}")
    used = qc.used_problems(probs)                   # asserts the condition
    left_out = {(c.name, q) for c, k, l, q, r in probs} - {(c.name, q) for c, k, l, q in used if k == "perturbed"}
    assert {n for n, _ in left_out} <= set(qc.MAY_BE_UNRESOLVED)
    assert all(r <= qc.RESOLVED_RTOL for c, k, l, q, r in probs if k == "converged")
    # on the default rule the four are exactly the ones the threshold drops, with a wide gap on either side of it.  The gap is
    # a property of the 64 x 21 rule only: on 200 x 21 perturbed norm12_R41 is kept at 3.8e-9, a factor 2.6 below the threshold, so
    # other multipliers may move it across -- which drops a named problem, as the condition allows
    res64 = {c.name: r for c, k, l, q, r in probs if k == "perturbed" and q == (64, 21)}
    assert {n for n, r in res64.items() if r > qc.RESOLVED_RTOL} == set(qc.MAY_BE_UNRESOLVED)
    assert min(r for r in res64.values() if r > qc.RESOLVED_RTOL) > 10 * qc.RESOLVED_RTOL
    assert max(r for r in res64.values() if r <= qc.RESOLVED_RTOL) < 0.1 * qc.RESOLVED_RTOL


def test_twin_calibration():
    """The fp64 twin of the quantile algorithm against the long-double reference over every used problem and the probability
    grid: its worst error per tolerance class stays at or below the recorded TWIN_UNITS_Q (which set the device tolerance), the
    quantiles are non-decreasing, the specials follow the convention."""
    worst = {}
    for case, kind, lam, quad in qc.used_problems(_problems()):
        x = qc.twin_quantiles(case, lam, quad, qc.GRID)
        assert np.all(np.diff(x) >= 0), (case.name, kind, quad)
        u = qc.quantile_units(qc.RuleTable(case, lam, quad), qc.GRID, x)
        k = int(np.argmax(u))
        cls = mc.tolerance_class(case)
        if u[k] > worst.get(cls, (-1.0, None))[0]:
            worst[cls] = (float(u[k]), f"{case.name} {kind} {quad[0]}x{quad[1]} p = {qc.GRID[k]:.6g}")
    print()
    for cls, (v, where) in sorted(worst.items()):
        print(f"twin quantiles: worst {cls:8s} {v:10.4g} units at {where} (recorded {qc.TWIN_UNITS_Q[cls]:g})")
    assert set(worst) == set(qc.TWIN_UNITS_Q)
    for cls, (v, where) in worst.items():
        assert v <= qc.TWIN_UNITS_Q[cls], (cls, v, where)
    case = mc.cases()["shifted_R6"]
    assert qc.quantile_tolerance(case) == 16.0 and qc.TWIN_UNITS_Q["shifted"] < 4.0       # the floor is the tolerance there
    assert qc.quantile_tolerance(mc.cases()["mix_R9"]) == 4.0 * qc.TWIN_UNITS_Q["regular"]
    case = mc.cases()["mix_R9"]
    lam = [l for c, k, l, q, r in _problems() if c.name == "mix_R9" and k == "converged" and q == (64, 21)][0]
    s = qc.twin_quantiles(case, lam, (64, 21), qc.SPECIALS)
    assert s[0] == case.domain[0] and s[1] == case.domain[1] and s[2] == case.domain[0] and np.all(np.isnan(s[3:]))


def test_reference_cdf_is_the_definition():
    """Fhat of the reference at the edges and ends: P_j / T at e_j, 0 at and below a, 1 at and above b, NaN for NaN; monotone on
    a resolved problem."""
    case = mc.cases()["mix_R9"]
    lam = [l for c, k, l, q, r in _problems() if c.name == "mix_R9" and k == "converged" and q == (64, 21)][0]
    ref = qc.RuleTable(case, lam, (64, 21))
    F, _ = ref.fhat(ref.e)
    assert F[0] == 0 and F[-1] == 1
    assert np.max(np.abs(F[1:-1] - ref.P[1:-1] / ref.T)) < 1e-18
    F, _ = ref.fhat([case.domain[0] - 1.0, case.domain[1] + 1.0, np.nan, -np.inf, np.inf])
    assert F[0] == 0 and F[1] == 1 and np.isnan(F[2]) and F[3] == 0 and F[4] == 1
    F, _ = ref.fhat(np.linspace(case.domain[0], case.domain[1], 1001))
    assert np.all(np.diff(F) > 0)


def test_entries_are_declared_bound_and_exported():
    from mlmc_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "mlmc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert name in text.split("#define MLMC_ABI_VERSION")[1].split("*/")[0], name + " is not named in the version comment"
    assert len(_lib.SIGNATURES["mlmc_density_integrate_batch"][1]) == 10
    assert len(_lib.SIGNATURES["mlmc_density_cdf_batch"][1]) == len(_lib.SIGNATURES["mlmc_density_quantiles_batch"][1]) == 14


def test_no_cpu_fallback_of_the_new_entries():
    """without a device the new Python entries raise like every other compute call"""
    import torch
    if torch.cuda.is_available():
        return
    from mlmc_amd import _lib, Legendre
    from mlmc_amd.tool import simple_distribution as sd
    from mlmc_amd.tool.distribution import Distribution
    dom = (-1.0, 1.0)
    data = np.stack([np.eye(4)[0], np.ones(4)], axis=1)
    d = sd.SimpleDistribution(Legendre(4, dom), data, domain=dom)
    d._initialize_params(4, 1e-8)
    for call in (lambda: sd.quantiles([d], [0.5]), lambda: sd.cdfs([d], [0.0]), lambda: sd.cdfs_on_rule([d], [0.0]),
                 lambda: d.quantile(0.5)):
        with pytest.raises(_lib.MlmcHipError):
            call()
    old = Distribution(Legendre(4, dom), data.copy(), domain=dom)
    old.multipliers, old._moment_errs = d.multipliers, d.moment_errs
    with pytest.raises(_lib.MlmcHipError):
        old.quantile([0.5])
    assert sd.quantiles([], [0.5]) == [] and sd.cdfs([], [0.5]) == [] and sd.cdfs_on_rule([], [0.5]) == []
