"""CPU tests of Genz's variable reordering: the NumPy twin of tests/box_order_cases.py against the permuted
covariance, against a long-double version of itself and on the named cases; what the order buys the chain on the project's own
Sobol' points; the argument errors of every new keyword and entry, which come before any device call; the new symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import box_order_cases as oc
from tests import box_prob_cases as bp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mlmc_copula_box_prob_pf_batch", "mlmc_copula_box_prob_t_pf_batch", "mlmc_copula_box_prob_tl_pf_batch",
               "mlmc_copula_box_order_batch")


@pytest.mark.parametrize("case", oc.ALL_CASES, ids=repr)
def test_twin_factors_the_permuted_covariance(case):
    t = oc.case_twin(case)
    assert t.ok.all() and oc.is_permutation(t.perm, case.M)
    want = oc.permuted_covariance(case.C, t.perm)
    got = t.L @ np.swapaxes(t.L, 1, 2)
    assert np.max(np.abs(got - want)) <= 8 * case.M * oc.U * np.max(np.abs(case.C))
    assert np.all(np.triu(t.L, 1) == 0.0) and np.all(np.diagonal(t.L, axis1=1, axis2=2) > 0.0)
    if case.first is not None:
        forced = case.first >= 0
        assert np.array_equal(t.perm[forced, 0], case.first[forced])


def test_named_permutations():
    assert np.array_equal(oc.case_twin(oc.ASC).perm[0], np.arange(12)[::-1])
    assert np.array_equal(oc.case_twin(oc.TIE).perm[0], np.arange(12))
    # the zero-width component has the smallest width there is: it leads, and its y is the edge nearer to 0
    zw = next(c for c in oc.SPECIAL_CASES if c.name == "zero-width")
    t = oc.case_twin(zw)
    assert np.all(t.perm[:, 0] == 2) and np.array_equal(t.y[:, 0], np.array([0.7, -0.4, 0.0]) / np.sqrt(zw.C[2, 2]))
    uf = next(c for c in oc.SPECIAL_CASES if c.name == "underflow")
    t = oc.case_twin(uf)
    assert np.all(t.perm[:, 0] == 1) and np.array_equal(t.y[:, 0], np.array([40.0, -40.0]))


def test_most_random_cases_have_clear_margins():
    """a condition on the case generator: the device's permutation is compared with the twin's only where no step is a near tie"""
    ok = [bool(oc.case_twin(c).qualifies().all()) for c in oc.RANDOM_CASES]
    print("\nrandom cases whose every step has a margin of {:g}: {} of {}".format(oc.MARGIN, sum(ok), len(ok)))
    assert sum(ok) >= 0.8 * len(ok)


LONG_DOUBLE_CASES = tuple(c for c in oc.ALL_CASES if c.B <= 3)


@pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="long double is not wider than double here")
def test_twin_against_its_long_double_version():
    worst = 0.0
    for case in LONG_DOUBLE_CASES:
        t = oc.case_twin(case)
        ref = oc.order_twin(case.C, case.lo, case.hi, case.shift, case.first, real=np.longdouble, forced_perm=t.perm)
        low = np.tril(np.ones((case.M, case.M), dtype=bool))[None] & (t.scale > 0)
        units = np.abs(t.L.astype(np.longdouble) - ref.L)[np.broadcast_to(low, t.L.shape)] / (oc.U * t.scale[np.broadcast_to(low, t.L.shape)])
        worst = max(worst, float(units.max()))
    print("\nthe twin's entries of L against long double: {:.2f} units (record {})".format(worst, oc.TWIN_UNITS_OBSERVED))
    assert worst <= oc.TWIN_UNITS_OBSERVED


@pytest.mark.parametrize("case,prototype", [(oc.ASC, 5.7128e-4), (oc.AR, 4.0e-8)], ids=["asc", "ar"])
def test_the_order_cuts_the_standard_error(case, prototype):
    """the chain twin on the project's own points, n = 2^12, 8 seeds: 10 x is the floor below which the feature would not be worth its
    code; what is measured goes to DESIGN.md 3.5.28"""
    (p_nat, se_nat, _), (p_ord, se_ord, _) = oc.natural_and_ordered(case, 2 ** 12)
    print("\n{}: natural {:.6g} +- {:.2g}, reordered {:.6g} +- {:.2g}: {:.0f} x".format(case, p_nat, se_nat, p_ord, se_ord, se_nat / se_ord))
    assert se_ord * 10.0 <= se_nat
    assert abs(p_nat - p_ord) <= 4.0 * np.hypot(se_nat, se_ord)
    assert abs(p_ord - prototype) <= 0.02 * prototype


# ---- argument errors: all of them before any device call (no device is bound in these tests) ------------------------------------
def _sd():
    from mlmc_amd.tool import simple_distribution
    return simple_distribution


def _uniform(M):
    from tests import score_cases as sk
    return [sk.closed_distribution(0.0, (0.0, 1.0)) for _ in range(M)]


def test_factor_shape_errors():
    sd = _sd()
    eye = np.eye(2)
    with pytest.raises(ValueError, match=r"square matrix \[M, M\] or one per box \[B, M, M\]"):
        sd.copula_box_probabilities(np.ones((1, 1, 2, 2)), 0.0, 1.0, 8, [0])
    with pytest.raises(ValueError, match=r"square matrix"):
        sd.copula_box_probabilities(np.ones(3), 0.0, 1.0, 8, [0])
    with pytest.raises(ValueError, match=r"factors must be \[B, M, M\]"):
        sd.copula_box_probabilities(np.ones((2, 3, 2)), 0.0, 1.0, 8, [0])
    with pytest.raises(ValueError, match="3 factors, one per box, but the limits hold 2 boxes"):
        sd.copula_box_probabilities(np.stack([eye] * 3), np.zeros((2, 2)), 1.0, 8, [0])
    bad = np.stack([eye, eye, eye])
    bad[1, 1, 1] = -1.0
    with pytest.raises(ValueError, match="box 1: the diagonal entry of factor row 1"):
        sd.copula_box_probabilities(bad, 0.0, 1.0, 8, [0])
    bad[1, 1, 1], bad[2, 1, 0] = 1.0, np.nan
    with pytest.raises(ValueError, match="box 2: factor row 1 has an entry that is not finite"):
        sd.copula_box_probabilities(bad, 0.0, 1.0, 8, [0], dof=3)
    with pytest.raises(ValueError, match="exceed the cap"):
        sd.copula_box_probabilities(np.stack([np.eye(129)] * 2), 0.0, 1.0, 8, [0])
    # the draws and the conditional t entries keep one shared factor
    with pytest.raises(ValueError, match="square matrix, got shape"):
        sd.copula_box_draws(np.stack([eye] * 2), 0.0, 1.0, 8, [0])
    with pytest.raises(ValueError, match="square matrix, got shape"):
        sd.conditional_box_probabilities(np.stack([eye] * 2), 0.0, 1.0, 8, [0], 3.0)


def test_box_order_errors():
    sd = _sd()
    c = oc.equicorrelation(3)
    for cov in (np.ones(3), np.ones((2, 3)), np.ones((1, 2, 3, 3))):
        with pytest.raises(ValueError, match=r"covariance must be \[M, M\] or one per box"):
            sd.box_order(cov, 0.0, 1.0)
    with pytest.raises(ValueError, match="exceed the cap"):
        sd.box_order(np.eye(129), 0.0, 1.0)
    with pytest.raises(ValueError, match="covariance must be finite"):
        sd.box_order(np.where(np.eye(3) > 0, np.nan, c), 0.0, 1.0)
    with pytest.raises(ValueError, match="2 covariances, one per box, but the limits hold 3 boxes"):
        sd.box_order(np.stack([c, c]), np.zeros((3, 3)), 1.0)
    with pytest.raises(ValueError, match="a limit of box 0, component 1 is NaN"):
        sd.box_order(c, [0.0, np.nan, 0.0], 1.0)
    with pytest.raises(ValueError, match="shift must be finite"):
        sd.box_order(c, 0.0, 1.0, shift=[0.0, np.inf, 0.0])
    with pytest.raises(ValueError, match="first of box 1 is 3"):
        sd.box_order(c, np.zeros((2, 3)), 1.0, first=[0, 3])
    with pytest.raises(ValueError, match="first of box 0 is -2"):
        sd.box_order(c, 0.0, 1.0, first=-2)
    with pytest.raises(ValueError, match="first must hold integers"):
        sd.box_order(c, 0.0, 1.0, first=0.5)
    with pytest.raises(ValueError, match="does not broadcast to the 2 boxes"):
        sd.box_order(c, np.zeros((2, 3)), 1.0, first=[0, 1, 2])


def test_order_keyword_errors():
    sd = _sd()
    d = _uniform(3)
    corr = oc.equicorrelation(3)
    kw = dict(n=8, seeds=[0], corr=corr)
    for entry in (sd.joint_probabilities, sd.event_samples):
        with pytest.raises(ValueError, match='order must be "natural" or "genz"'):
            entry(d, 0.2, 0.8, order="pivoted", **kw)
    with pytest.raises(ValueError, match='order must be "natural" or "genz"'):
        sd.conditional_probabilities(d, 0.2, 0.8, {0: 0.5}, order=None, **kw)
    with pytest.raises(ValueError, match='order="genz" is out of scope here: a conditional law of the t copula'):
        sd.conditional_probabilities(d, 0.2, 0.8, {0: 0.5}, dof=3, order="genz", **kw)
    with pytest.raises(ValueError, match='order="genz" is out of scope here: the draws entries'):
        sd.event_samples(d, 0.2, 0.8, order="genz", **kw)
    with pytest.raises(ValueError, match='order="genz" is out of scope here: the draws entries'):
        sd.conditional_event_samples(d, 0.2, 0.8, {0: 0.5}, order="genz", **kw)
    with pytest.raises(ValueError, match='order must be "natural" or "genz"'):
        sd.joint_probabilities_over_correlations(d, 0.2, 0.8, 8, [0], corr[None], order="best")
    with pytest.raises(ValueError, match=r"corrs must be \[C, M, M\]"):
        sd.joint_probabilities_over_correlations(d, 0.2, 0.8, 8, [0], corr)
    # a call that constrains nothing needs no device: ones, and an empty order
    res, perm = sd.joint_probabilities(d, -np.inf, np.inf, order="genz", return_order=True, **kw)
    assert np.array_equal(res.prob, [1.0]) and perm.shape == (1, 0)
    res, ok = sd.joint_probabilities_over_correlations(d, -np.inf, np.inf, 8, [0], np.stack([corr, corr]), order="genz")
    assert ok.all() and len(res) == 2 and np.array_equal(res[1].prob, [1.0])


def test_estimate_order_keyword_errors():
    from mlmc_amd.estimator import Estimate
    from tests.test_gpu_bootstrap_batch import _levels, _memory, _root_q
    st = _memory(_levels([60, 30], 3, nan=False), 3)
    e = Estimate(_root_q(st, 3), st)
    for call in (lambda: e.estimate_joint_probability(-1.0, 1.0, order="x"), lambda: e.estimate_joint_exceedance(0.0, order="x"),
                 lambda: e.bootstrap_joint_probability(-1.0, 1.0, 4, order="x"), lambda: e.bootstrap_joint_exceedance(0.0, 4, order="x")):
        with pytest.raises(ValueError, match='order must be "natural" or "genz"'):
            call()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_named():
    from mlmc_amd import _lib
    header = open(os.path.join(ROOT, "include", "mlmc_hip.h")).read()
    version_comment = header[header.index("#define MLMC_ABI_VERSION"):header.index("/* basis kinds")]
    assert re.search(r"#define MLMC_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert name in version_comment, name
        assert re.search(r"\bint " + name + r"\(", header), name
    so = os.path.join(ROOT, "mlmc_amd", "libmlmc_hip.so")
    lib = ctypes.CDLL(so)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.mlmc_abi_version() == 8
    # the stride sits behind the factor in every per-box entry
    for name in NEW_SYMBOLS[:3]:
        assert _lib.SIGNATURES[name][1][2] is ctypes.c_int64
        old = _lib.SIGNATURES[name.replace("_pf_batch", "_batch")][1]
        assert _lib.SIGNATURES[name][1][:2] + _lib.SIGNATURES[name][1][3:] == old
