"""CPU tests of the divergences between max-entropy densities: the calibration of the fp64 twin against the long-double reference
(tests/divergence_cases.py), the reference against identities of its own definition, the boundary of the new entry (declared,
bound, exported, ABI version unchanged), the argument checks of `divergences` that come before any device call, and the
percentile helper of Estimate.bootstrap_component_divergences."""
import os
import re

import numpy as np
import pytest

from tests import divergence_cases as dc
from tests import maxent_cases as mc
from tests import quantile_cases as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "mlmc_density_divergences_batch"
LD = np.longdouble

_TABLE = None


def _table():
    """the pair table at fp64 Newton multipliers with reference and twin (the device is not involved)"""
    global _TABLE
    if _TABLE is None:
        _TABLE = [(p,) + p.reference() + (p.reference(np.float64)[0],) for p in dc.pairs()]
    return _TABLE


def test_pair_table():
    tags = [p.tag for p, _, _, _ in _table()]
    n_cases = len(mc.cases())
    assert len(tags) == len(set(tags)) == len(qc.RULES) * (3 * n_cases + len(dc.SELF_CASES) + len(dc.CROSS) + len(dc.G6_CROSS))
    for quad in qc.RULES:
        rule = f" {quad[0]}x{quad[1]}"
        for name in mc.cases():
            assert f"{name} converged / perturbed{rule}" in tags and f"{name} converged / scaled 1+1e-06{rule}" in tags
        assert f"log_legendre_R8 converged / perturbed{rule}" in tags and f"shifted_R6 converged / scaled 1+0.01{rule}" in tags
    classes = {p.cls for p, _, _, _ in _table()}
    assert classes == set(dc.TWIN_UNITS_D) == {"regular", "shifted"}
    kinds = [{p.prior[0].desc.kind, p.posterior[0].desc.kind} for p, _, _, _ in _table()]
    assert {"legendre", "fourier"} in kinds and {"monomial", "spline"} in kinds
    crossed = [p for p, _, _, _ in _table() if "intersection" in p.tag]
    assert crossed and all(p.interval not in (p.prior[0].domain, p.posterior[0].domain) or p.prior[0].domain != p.posterior[0].domain
                           for p in crossed)
    assert any(p.interval != p.prior[0].domain and p.interval != p.posterior[0].domain for p in crossed)


def test_twin_calibration():
    """The fp64 twin against the long-double reference over the whole pair table, every column: the worst error per tolerance
    class stays at or below the recorded TWIN_UNITS_D, which set the device tolerance."""
    worst = {}
    for p, ref, scale, twin in _table():
        u = dc.units(twin, ref, scale)
        for c in range(6):
            key = (p.cls, dc.COLUMNS[c])
            if u[c] > worst.get(key, (-1.0, None))[0]:
                worst[key] = (float(u[c]), p.tag)
    print()
    for (cls, col), (v, where) in sorted(worst.items()):
        print(f"twin divergences: worst {cls:8s} {col:7s} {v:10.4g} units at {where} (recorded {dc.TWIN_UNITS_D[cls]:g})")
    for (cls, col), (v, where) in worst.items():
        assert v <= dc.TWIN_UNITS_D[cls], (cls, col, v, where)
    for cls in dc.TWIN_UNITS_D:                                     # the record is the measurement, not a generous bound
        assert max(v for (c, _), (v, _) in worst.items() if c == cls) >= 0.9 * dc.TWIN_UNITS_D[cls], cls
        assert dc.divergence_tolerance(cls) == max(16.0, 4.0 * dc.TWIN_UNITS_D[cls])
    # the small-d regime: a KL scale without its |d| term would put these pairs at thousands of units
    small = [dc.units(twin, ref, scale)[:4].max() for p, ref, scale, twin in _table() if "scaled 1+1e-06" in p.tag and p.cls == "regular"]
    assert len(small) == 2 * (len(mc.cases()) - 1) and max(small) <= 16.0, max(small)


def test_reference_identities():
    for p, ref, scale, twin in _table():
        assert np.all(np.isfinite(ref)) and np.all(scale[4:] > 0), p.tag
        if p.same:                      # exact zeros and equal masses, in both precisions (mix_R1: perturbed(lam) is lam itself)
            assert np.all(ref[:4] == 0) and ref[dc.MASS_P] == ref[dc.MASS_Q], p.tag
            assert np.all(twin[:4] == 0) and twin[dc.MASS_P] == twin[dc.MASS_Q], p.tag
        else:
            assert np.all(ref[:4] > 0) and np.all(scale[:4] > 0), p.tag
        # (sqrt q - sqrt p)^2 <= |q - p| at every node, hence H2 <= TV; TV <= (mass_p + mass_q) / 2; Cauchy-Schwarz 2 TV <= sqrt(L2SQ width)
        assert ref[dc.H2] <= ref[dc.TV] <= (ref[dc.MASS_P] + ref[dc.MASS_Q]) / 2 * (1 + LD(1e-15)), p.tag
        width = LD(p.interval[1]) - LD(p.interval[0])
        assert 2 * ref[dc.TV] <= np.sqrt(ref[dc.L2SQ] * width) * (1 + LD(1e-15)), p.tag
        # the masses on the whole domain are the masses of the quantile checks' table (summed in another order)
        for (case, lam), col in ((p.prior, dc.MASS_P), (p.posterior, dc.MASS_Q)):
            if p.interval == case.domain:
                assert abs(ref[col] - qc.RuleTable(case, lam, p.quad).T) <= 256 * np.finfo(LD).eps * ref[col], p.tag


def test_reference_specials():
    case = mc.cases()["mix_R9"]
    lam = [p.prior[1] for p, _, _, _ in _table() if p.tag == "mix_R9 / itself 64x21"][0]
    # NaN multipliers and an interval that leaves the basis' domain: six NaNs
    bad = lam.copy()
    bad[3] = np.nan
    assert np.all(np.isnan(dc.pair_sums((case, lam), (case, bad), case.domain, (64, 21))[0]))
    assert np.all(np.isnan(dc.pair_sums((case, lam), (case, lam), (case.domain[0] - 1.0, case.domain[1]), (64, 21))[0]))
    # oppositely clipped exponents: x^2 leaves the fp64 range, L2SQ alone is inf, in the long-double reference too
    lc = mc.clip_multipliers(case, lam)
    exps = []
    vals, _ = dc.pair_sums((case, lc), (case, -lc), case.domain, (64, 21), exponents=exps)
    mc.assert_clip_band(exps[0])
    mc.assert_clip_band(exps[1])
    dc.assert_overflow_band(exps[2])
    assert np.max(exps[2]) == 400 and np.min(exps[2]) == -400
    assert np.isinf(vals[dc.L2SQ]) and np.all(np.isfinite(np.delete(vals, dc.L2SQ)))
    twin, _ = dc.pair_sums((case, lc), (case, -lc), case.domain, (64, 21), np.float64)
    assert np.isinf(twin[dc.L2SQ]) and np.all(np.isfinite(np.delete(twin, dc.L2SQ)))


def test_entry_is_declared_bound_and_exported():
    from mlmc_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "mlmc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+" + ENTRY + r"\s*\(", code)
    assert ENTRY in _lib.SIGNATURES and hasattr(lib, ENTRY)
    comment = text.split("#define MLMC_ABI_VERSION")[1].split("*/")[0]
    assert ENTRY in comment.split("added within 8")[1], ENTRY + " is not named in the version comment"
    assert len(_lib.SIGNATURES[ENTRY][1]) == 15
    assert _lib.ABI_VERSION == 8 and lib.mlmc_abi_version() == 8
    assert re.search(r"#define\s+MLMC_ABI_VERSION\s+8\b", text)
    for c, name in enumerate(("KL", "L2SQ", "TV", "H2", "MASS_P", "MASS_Q", "COUNT")):
        assert re.search(r"\bMLMC_DIV_" + name + r"\s*=\s*" + str(c) + r"\b", code), name


def _toy(cls=None, dom=(-1.0, 1.0)):
    from mlmc_amd import Legendre
    from mlmc_amd.tool import simple_distribution as sd
    cls = sd.SimpleDistribution if cls is None else cls
    d = cls(Legendre(4, dom), np.stack([np.eye(4)[0], np.ones(4)], axis=1), domain=dom)
    d.multipliers, d._moment_errs = np.array([np.log(dom[1] - dom[0]), 0.0, 0.0, 0.0]), np.ones(4)
    return d


def test_divergences_checks_before_any_device_call(monkeypatch):
    from mlmc_amd import _lib
    from mlmc_amd.tool import simple_distribution as sd
    from mlmc_amd.tool.distribution import Distribution

    def no_device():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_device)
    res = sd.divergences([], [])
    assert isinstance(res, sd.Divergences) and res._fields == ("kl", "l2", "tv", "hellinger", "mass_prior", "mass_posterior")
    assert all(isinstance(v, np.ndarray) and v.shape == (0,) for v in res)
    d, e = _toy(), _toy()
    with pytest.raises(ValueError, match="divergences: 2 priors for 1 posteriors"):
        sd.divergences([d, d], [e])
    far = _toy(dom=(3.0, 4.0))
    with pytest.raises(ValueError, match="divergences: pair 1: the two domains do not intersect"):
        sd.divergences([d, d], [e, far])
    touching = _toy(dom=(1.0, 2.0))
    with pytest.raises(ValueError, match="pair 0: the two domains do not intersect"):
        touching.divergence(d)
    other = _toy()
    other.n_intervals = 200
    with pytest.raises(ValueError, match="divergences: every distribution must use the same quadrature"):
        sd.divergences([d], [other])
    other = _toy(Distribution)
    other._gauss_degree = 5
    with pytest.raises(ValueError, match="every distribution must use the same quadrature"):
        other.divergence(d)
    with pytest.raises(ValueError, match="intervals must be one"):
        sd.divergences([d, d], [e, e], intervals=[(0.0, 1.0)] * 3)


def test_no_cpu_fallback_of_the_new_entries():
    import torch
    from mlmc_amd import _lib, estimator
    from mlmc_amd.tool import simple_distribution as sd
    from mlmc_amd.tool.distribution import Distribution
    assert callable(estimator.Estimate.bootstrap_component_divergences)
    with pytest.raises(ValueError, match="bootstrap_component_divergences: level must be"):
        estimator.Estimate(None, None, None).bootstrap_component_divergences(4, level=1.0)
    if torch.cuda.is_available():
        return
    d, e, old = _toy(), _toy(), _toy(Distribution)
    for call in (lambda: sd.divergences([d], [e]), lambda: e.divergence(d), lambda: old.divergence(d, interval=(-0.5, 0.5))):
        with pytest.raises(_lib.MlmcHipError):
            call()


def test_divergence_upper():
    from mlmc_amd.estimator import DivergenceSpread, divergence_upper
    assert DivergenceSpread._fields == ("kl", "l2", "tv", "hellinger", "upper", "success", "n_ok", "seed")
    rng = np.random.default_rng(5)
    B, M = 40, 3
    measures = [rng.random((B, M)) * (k + 1) for k in range(4)]
    success = rng.random((B, M)) < 0.8
    success[:, 1] = False                                           # a component without a successful replicate
    success[:, 2] = True
    measures[0][~success] = np.nan                                  # what a failed replicate may leave behind
    upper = divergence_upper(measures, success, 0.9)
    assert upper.shape == (M, 4) and np.all(np.isnan(upper[1])) and np.all(np.isfinite(upper[[0, 2]]))
    for m in (0, 2):
        for k in range(4):
            assert upper[m, k] == np.percentile(measures[k][success[:, m], m], 90.0), (m, k)
    assert np.array_equal(upper[2], [np.percentile(v[:, 2], 90.0) for v in measures])
    one = divergence_upper([v[:1] for v in measures], np.ones((1, M), dtype=bool), 0.5)
    assert np.array_equal(one[2], [v[0, 2] for v in measures])
    for level in (0.0, 1.0, True, "0.9", None):
        with pytest.raises(ValueError, match="divergence_upper: level must be"):
            divergence_upper(measures, success, level)
    with pytest.raises(ValueError, match="divergence_upper: four measures"):
        divergence_upper(measures[:3], success, 0.9)
    with pytest.raises(ValueError, match="divergence_upper: four measures"):
        divergence_upper(measures, success[:, :2], 0.9)
