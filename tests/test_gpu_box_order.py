"""GPU tests of Genz's variable reordering and of the chain with one factor per box, at the level of the C entries:
mlmc_copula_box_order_batch against the NumPy twin of tests/box_order_cases.py on every case, and the _pf_ entries
(mlmc_copula_box_prob_pf_batch, _t_pf_batch, _tl_pf_batch) against the entries with one shared factor bit for bit, against single-box
calls bit for bit and against the chain twin of tests/box_prob_cases.py per point."""
import functools
import re

import numpy as np
import pytest

from tests import box_order_cases as oc
from tests import box_prob_cases as bp
from tests.test_gpu_joint_samples import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
U = bp.U


def _sd():
    from mlmc_amd.tool import simple_distribution
    return simple_distribution


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@functools.lru_cache(maxsize=None)
def _device_order(case):
    return _sd().box_order(case.C, case.lo, case.hi, shift=case.shift, first=case.first, check=False)


# ---- the order kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", oc.ALL_CASES, ids=repr)
def test_order_against_the_twin(hip, case):
    got, t = _device_order(case), oc.case_twin(case)
    B, M = case.B, case.M
    assert got.perm.shape == (B, M) and got.perm.dtype == np.int32 and got.factor.shape == (B, M, M) and got.ok.shape == (B,)
    assert got.ok.all()
    assert oc.is_permutation(got.perm, M)
    clear = t.qualifies()
    assert np.array_equal(got.perm[clear], t.perm[clear])
    agree = np.all(got.perm == t.perm, axis=1)
    print("\n{}: {} of {} boxes with clear margins, {} with the twin's permutation".format(case, int(clear.sum()), B, int(agree.sum())))
    # the factor: within the tolerance of the twin wherever the permutation is the twin's
    err = np.abs(got.factor - t.L)[agree]
    tol = U * oc.GPU_TOLERANCE_UNITS * t.scale[agree]
    assert np.all(err <= tol)
    worst = float(np.max(err / np.where(t.scale[agree] > 0, U * t.scale[agree], 1.0))) if agree.any() else 0.0
    print("factor against the twin: {:.3g} units (tolerance {:.4g})".format(worst, oc.GPU_TOLERANCE_UNITS))
    # ... and a factor of the permuted covariance in every box
    want = oc.permuted_covariance(case.C, got.perm)
    assert np.max(np.abs(got.factor @ np.swapaxes(got.factor, 1, 2) - want)) <= 8 * M * U * np.max(np.abs(case.C))
    assert np.all(np.triu(got.factor, 1) == 0.0) and np.all(np.diagonal(got.factor, axis1=1, axis2=2) > 0.0)
    # limits and shift come back permuted
    at = got.perm.astype(np.int64)
    assert _same(got.lower, np.take_along_axis(case.lo, at, axis=1)) and _same(got.upper, np.take_along_axis(case.hi, at, axis=1))
    assert (got.shift is None) == (case.shift is None)
    if case.shift is not None:
        assert _same(got.shift, np.take_along_axis(case.shift, at, axis=1))
    if case.first is not None:
        forced = case.first >= 0
        assert np.array_equal(got.perm[forced, 0], case.first[forced])


def test_named_orders(hip):
    assert np.array_equal(_device_order(oc.ASC).perm[0], np.arange(12)[::-1])
    assert np.array_equal(_device_order(oc.TIE).perm[0], np.arange(12))


@pytest.mark.parametrize("case", [c for c in oc.ALL_CASES if c.C.ndim == 2 and c.B in (3, 70) and c.M in (3, 5, 65, 128)], ids=repr)
def test_shared_covariance_equals_copies_and_repeats(hip, case):
    sd = _sd()
    shared = _device_order(case)
    copies = sd.box_order(np.stack([case.C] * case.B), case.lo, case.hi, shift=case.shift, first=case.first, check=False)
    again = sd.box_order(case.C, case.lo, case.hi, shift=case.shift, first=case.first, check=False)
    for other in (copies, again):
        assert np.array_equal(other.perm, shared.perm) and _same(other.factor, shared.factor) and np.array_equal(other.ok, shared.ok)
    # a box does not depend on its position or on the batch
    b = case.B - 1
    alone = sd.box_order(case.C, case.lo[b], case.hi[b], shift=None if case.shift is None else case.shift[b],
                         first=None if case.first is None else case.first[b:], check=False)
    assert np.array_equal(alone.perm[0], shared.perm[b]) and _same(alone.factor[0], shared.factor[b])


def test_padded_stride_and_errors_of_the_order_entry(hip):
    case = next(c for c in oc.SPECIAL_CASES if c.name == "stride")
    B, M = case.B, case.M
    want = _device_order(case)

    def raw(C, stride, lo=case.lo, hi=case.hi, M=M, B=B, shift=None, first=None):
        C, lo, hi = (np.ascontiguousarray(x, dtype=np.float64) for x in (C, lo, hi))
        perm, L, ok = np.full((B, max(M, 1)), -7, dtype=np.int32), np.empty((B, max(M, 1), max(M, 1))), np.zeros(B, dtype=np.int32)
        shift = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
        first = None if first is None else np.ascontiguousarray(first, dtype=np.int32)
        rc = hip.lib().mlmc_copula_box_order_batch(M, hip.ptr(C), stride, B, hip.ptr(lo), hip.ptr(hi), hip.ptr(shift), hip.ptr(first),
                                                   hip.ptr(perm), hip.ptr(L), hip.ptr(ok))
        return rc, perm, L, ok, hip.lib().mlmc_last_error().decode()

    padded = np.full((B, M * M + 5), np.nan)
    padded[:, :M * M] = case.C.reshape(B, M * M)
    rc, perm, L, ok, _ = raw(padded, M * M + 5)
    assert rc == 0 and np.array_equal(perm, want.perm) and _same(L, want.factor) and ok.all()
    nan_lo = case.lo.copy()
    nan_lo[1, 2] = np.nan
    bad_c = case.C.copy()
    bad_c[2, 1, 3] = np.inf
    for kw, match in ((dict(stride=M * M - 1), "cov_stride = 35 must be 0 .* or at least M \\* M = 36"),
                      (dict(stride=-1), "cov_stride"),
                      (dict(M=0), "M < 1"),
                      (dict(M=129), "cap"),
                      (dict(B=0), "B < 1"),
                      (dict(lo=nan_lo), "box 1, component 2: a limit is NaN"),
                      (dict(C=bad_c), "box 2, covariance row 1: entry 3 is not finite"),
                      (dict(shift=np.where(np.arange(B * M).reshape(B, M) == 7, np.inf, 0.0)), "box 1, component 1: the shift is not finite"),
                      (dict(first=[0, M, -1]), "box 1: first = 6"),
                      (dict(first=[0, -2, -1]), "box 1: first = -2")):
        args = dict(C=case.C, stride=M * M)
        args.update(kw)
        rc, perm, _, _, msg = raw(**args)
        assert rc != 0 and re.search(match, msg) and msg.startswith("mlmc_copula_box_order_batch:"), (kw, msg)
        assert np.all(perm == -7)
    # a covariance that is not positive definite: ok is cleared for that box alone, perm stays a permutation, Python names the box
    C = np.stack([oc.equicorrelation(3), np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), oc.equicorrelation(3)])
    res = _sd().box_order(C, -1.0, 1.0, check=False)
    assert res.ok.tolist() == [True, False, True] and oc.is_permutation(res.perm, 3)
    with pytest.raises(ValueError, match="box 1: the covariance is not positive definite"):
        _sd().box_order(C, -1.0, 1.0)


# ---- the chain with one factor per box ------------------------------------------------------------------------------------------
MODES = (dict(), dict(dof=3.0), dict(dof=3.0, mixing="conditioned"))
MODE_IDS = ("gauss", "t", "lead")


def _problem(M, B, seed=0):
    """B different factors [B, M, M], limits [B, M]"""
    lo, hi = bp.boxes(M, B, 300 + M + seed)
    return np.stack([bp.chol_factor(M, 400 + 10 * M + b + seed) for b in range(B)]), lo, hi


def _call(L, lo, hi, mode, n=200, seeds=(3, 11), first=37, **kw):
    more = dict(return_mixing=True) if "dof" in mode else {}
    if mode.get("mixing") == "conditioned":
        more["return_lead"] = True
    return _sd().copula_box_probabilities(L, lo, hi, n, list(seeds), first=first, return_integrand=True, **mode, **more, **kw)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("M", [1, 2, 12, 65])
@pytest.mark.parametrize("B", [1, 3])
def test_copies_of_one_factor_equal_the_shared_call(hip, mode, M, B):
    Ls, lo, hi = _problem(M, B)
    n = 200 if M < 65 else 70
    shared = _call(Ls[0], lo, hi, mode, n=n)
    copies = _call(np.stack([Ls[0]] * B), lo, hi, mode, n=n)
    assert len(shared) == len(copies)
    assert _same(shared[0].replicates, copies[0].replicates) and _same(shared[0].prob, copies[0].prob)
    for a, b in zip(shared[1:], copies[1:]):
        assert _same(a, b)
    if not mode:                                       # the Gaussian entry takes a shift
        sh = np.random.default_rng(M).uniform(-0.5, 0.5, (B, M))
        a, b = _call(Ls[0], lo, hi, mode, n=n, shift=sh), _call(np.stack([Ls[0]] * B), lo, hi, mode, n=n, shift=sh)
        assert _same(a[0].replicates, b[0].replicates) and _same(a[1], b[1])


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("M", [1, 2, 12, 65])
def test_different_factors_equal_single_box_calls(hip, mode, M):
    B = 3
    Ls, lo, hi = _problem(M, B, seed=1)
    n = 200 if M < 65 else 70
    for qmc in (True, False):
        batch = _call(Ls, lo, hi, mode, n=n, qmc=qmc)
        assert batch[0].replicates.shape == (2, B) and batch[1].shape == (2, B, n)
        for b in range(B):
            one = _call(Ls[b], lo[b], hi[b], mode, n=n, qmc=qmc)
            assert _same(batch[0].replicates[:, b], one[0].replicates[:, 0]) and _same(batch[1][:, b], one[1][:, 0])
            if mode.get("mixing") == "conditioned":
                assert _same(batch[2][:, b], one[2][:, 0]) and _same(batch[3][:, b], one[3][:, 0])
            elif mode:
                assert _same(batch[2], one[2])          # the mixing scales do not depend on the box
    if M > 1:
        assert not _same(batch[1][:, 0], _call(Ls[1], lo[0], hi[0], mode, n=n, qmc=False)[1][:, 0])


@pytest.mark.parametrize("M,n,first,qmc", [(2, 65, 0, True), (5, 63, 777, False), (17, 33, 4095, True), (65, 17, 0, True)])
def test_per_box_integrand_against_the_twin(hip, M, n, first, qmc):
    B, seeds = 3, (2, 9)
    Ls, lo, hi = _problem(M, B, seed=2)
    sh = np.random.default_rng(5 * M).uniform(-1.0, 1.0, (B, M))
    res, f = _sd().copula_box_probabilities(Ls, lo, hi, n, list(seeds), shift=sh, first=first, qmc=qmc, return_integrand=True)
    worst = 0.0
    for r, seed in enumerate(seeds):
        w = bp.points(seed, list(range(M - 1)), first, n, qmc)
        for b in range(B):
            want, scale = bp.twin(Ls[b], lo[b], hi[b], sh[b], w)
            ok = want > 0
            assert np.all(f[r, b][~ok] == 0.0)
            units = np.abs(f[r, b][ok] - want[ok]) / (U * scale[ok] * want[ok])
            worst = max(worst, float(units.max()) if ok.any() else 0.0)
            assert res.replicates[r, b] == bp.tree_mean(f[r, b], first, M)
    print("\nper-box integrand against the twin, M = {}: {:.3g} units (tolerance {})".format(M, worst, bp.GPU_TOLERANCE_UNITS))
    assert worst <= bp.GPU_TOLERANCE_UNITS


def test_padded_factor_stride_and_errors(hip):
    M, B, n = 3, 3, 64
    Ls, lo, hi = _problem(M, B, seed=3)
    seeds = np.array([4], dtype=np.uint64)
    want = _sd().copula_box_probabilities(Ls, lo, hi, n, [4]).replicates

    def raw(name, L, stride, dof=None, lo=lo):
        L, lo_, hi_ = (np.ascontiguousarray(x, dtype=np.float64) for x in (L, lo, hi))
        mean = np.full((1, B), -7.0)
        fn = getattr(hip.lib(), name)
        if dof is None:
            rc = fn(M, hip.ptr(L), stride, B, hip.ptr(lo_), hip.ptr(hi_), None, 1, hip.ptr(seeds), None, 0, n, 8, hip.ptr(mean), None, 0)
        elif name.endswith("tl_pf_batch"):
            rc = fn(M, hip.ptr(L), stride, B, hip.ptr(lo_), hip.ptr(hi_), dof, 1, hip.ptr(seeds), None, 7, 0, n, 8, hip.ptr(mean), None,
                    None, None, 0)
        else:
            rc = fn(M, hip.ptr(L), stride, B, hip.ptr(lo_), hip.ptr(hi_), dof, 1, hip.ptr(seeds), None, 7, 0, n, 8, hip.ptr(mean), None,
                    None, 0)
        return rc, mean, hip.lib().mlmc_last_error().decode()

    padded = np.full((B, M * M + 7), np.nan)
    padded[:, :M * M] = Ls.reshape(B, M * M)
    rc, mean, _ = raw("mlmc_copula_box_prob_pf_batch", padded, M * M + 7)
    assert rc == 0 and _same(mean, want)
    # stride 0: the entry with one shared factor
    rc, mean, _ = raw("mlmc_copula_box_prob_pf_batch", Ls[0], 0)
    assert rc == 0 and _same(mean, _sd().copula_box_probabilities(Ls[0], lo, hi, n, [4]).replicates)
    bad = Ls.copy()
    bad[2, 1, 1] = 0.0
    nan = Ls.copy()
    nan[1, 2, 0] = np.nan
    for name, dof in (("mlmc_copula_box_prob_pf_batch", None), ("mlmc_copula_box_prob_t_pf_batch", 3.0),
                      ("mlmc_copula_box_prob_tl_pf_batch", 3.0)):
        for args, match in (((Ls, M * M - 1), "factor_stride = 8 must be 0 .* or at least M \\* M = 9"),
                            ((Ls, -9), "factor_stride"),
                            ((bad, M * M), "box 2, factor row 1: the diagonal entry must be finite and positive"),
                            ((nan, M * M), "box 1, factor row 2: entry 0 is not finite")):
            rc, mean, msg = raw(name, *args, dof=dof)
            assert rc != 0 and re.search(match, msg) and msg.startswith(name + ":"), (name, msg)
            assert np.all(mean == -7.0)
        # the upper part of a factor is ignored, as with one shared factor
        upper = Ls + np.triu(np.full((M, M), np.nan), 1)[None]
        assert raw(name, upper, M * M, dof=dof)[0] == 0
