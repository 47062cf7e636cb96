"""GPU checks of the two fp64 matrix-core contractions against the 80-bit long-double reference of tests/gram_exact.py, in units
of 2^-53 * (condition scale): the component covariance (k_xcov_mask, k_xcov_accum, k_xcov_reduce) through
engine.ComponentCovAccumulator, and the bootstrap contraction (k_bs_keep, k_bs_keep_multi, k_bs_contract, k_bs_reduce) through
engine.BootstrapAccumulator and engine.ComponentBootstrapAccumulator.  Cases and tolerances are those of tests/gram_cases.py:
the tolerance of a class is max(16, 4 x the worse of the two fp64 twins), calibrated without a device by
tests/test_gram_exact_cpu.py.  No entry, replicate or case is left out of a comparison; a zero scale demands an exact zero; a
non-finite device value fails except where the contract says NaN (sp of a mean-only accumulator).  Every test prints its worst
units with the case, level, entry and replicate where they occur (pytest -s)."""
import numpy as np
import pytest

from tests import accum_exact as ax
from tests import gram_cases as gc

pytestmark = pytest.mark.gpu

WEIGHT_BLOCK = 1 << 20                    # weights fetched at a time for the kept counts of every replicate: never B x n


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


class Worst:
    """the worst units of a test per quantity, with the place; the entries over their tolerance (a test prints all its figures
    before it fails)"""

    def __init__(self):
        self.w = {}
        self.failures = []

    def check(self, ok, *what):
        if not ok:
            self.failures.append(what)

    def add(self, q, units, tol, place):
        if q not in self.w or units / tol > self.w[q][0] / self.w[q][1]:
            self.w[q] = (units, tol, place)
        self.check(units <= tol, q, units, tol, place)

    def show(self, title):
        print()
        for q, (units, tol, place) in sorted(self.w.items()):
            print("{:14s} {:22s} worst {:10.4g} units (tolerance {:.4g})  at {}".format(title, q, units, tol, place))


# ---------------------------------------------------------------------------------------------------------------------------
# component covariance
# ---------------------------------------------------------------------------------------------------------------------------
def _xcov_device(case, mean_only=False, ragged=False):
    """whole levels from host arrays, or every level in ragged chunks from device tensors -> n, n_rm, s, sp"""
    import torch
    from mlmc_amd.engine import ComponentCovAccumulator
    acc = ComponentCovAccumulator(case.M, case.L, mean_only=mean_only)
    acc.set_shift(case.shift)
    for l, (f, c) in enumerate(case.levels):
        n = f.shape[1]
        cuts = gc.ragged_cuts(n) if ragged else [0, n]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            fb = np.ascontiguousarray(f[:, lo:hi])
            cb = None if c is None else np.ascontiguousarray(c[:, lo:hi])
            if ragged:
                fb = torch.from_numpy(fb).cuda()
                cb = None if cb is None else torch.from_numpy(cb).cuda()
            acc.push(l, fb, cb)
    out = acc.finalize()
    acc.close()
    return out


def _xcov_judge(case, got, label, worst, mean_only=False):
    ref, M = gc.xcov_reference(case), case.M
    n, n_rm, s, sp = got
    assert np.array_equal(n, ref.n) and np.array_equal(n_rm, ref.n_rm), (case, label, n, ref.n, n_rm, ref.n_rm)
    assert s.shape == ref.s.shape and sp.shape == ref.sp.shape
    for l, (f, c) in enumerate(case.levels):
        cls = gc.xcov_class(M, c is not None)
        S = s[l].reshape(M, M)
        worst.check(np.array_equal(S, S.T), "s is not bitwise symmetric", case, label, l)
        quantities = [("s", s[l], ref.s[l], ref.S[l])]
        if mean_only:
            worst.check(bool(np.all(np.isnan(sp[l]))), "sp of a mean-only accumulator is not NaN", case, label, l)
        else:
            SPm = sp[l].reshape(M, M)
            worst.check(np.array_equal(SPm, SPm.T), "sp is not bitwise symmetric", case, label, l)
            quantities.append(("sp", sp[l], ref.sp[l], ref.SP[l]))
        for q, value, want, scale in quantities:
            units, flat = ax.worst(value, want, scale)
            worst.add("{} {}".format(cls, q), units, gc.xcov_tolerance(cls, q),
                      "{} [{}] level {} (n = {}) entry ({}, {})".format(case.name, label, l, f.shape[1], flat // M, flat % M))


XCOV_GROUPS = {}
for _case in gc.xcov_cases().values():
    _key = _case.name.split("_")[0] if _case.name.split("_")[0] in ["m{}".format(M) for M in gc.XCOV_M + (1024,)] else "special"
    XCOV_GROUPS.setdefault(_key, []).append(_case)


@pytest.mark.parametrize("group", list(XCOV_GROUPS))
def test_component_covariance_against_the_long_double_reference(hip, group):
    """Every case of one M (or the special cases): one push per level, the same levels in ragged chunks from device tensors, and
    the mean-only accumulator -- each held to the reference on its own: counts exactly, every entry of s and sp in units of its
    scale, exact zeros where the scale is zero, bitwise symmetry, sp = NaN and s unchanged under mean_only."""
    worst = Worst()
    for case in XCOV_GROUPS[group]:
        whole = _xcov_device(case)
        _xcov_judge(case, whole, "whole", worst)
        _xcov_judge(case, _xcov_device(case, ragged=True), "ragged", worst)
        mean = _xcov_device(case, mean_only=True)
        _xcov_judge(case, mean, "mean_only", worst, mean_only=True)
    worst.show(group)
    assert not worst.failures, worst.failures[:8]


# ---------------------------------------------------------------------------------------------------------------------------
# bootstrap
# ---------------------------------------------------------------------------------------------------------------------------
def _fn(desc):
    from mlmc_amd import Fourier, Legendre, Monomial
    cls = {ax.LEGENDRE: Legendre, ax.MONOMIAL: Monomial, ax.FOURIER: Fourier}[desc.kind]
    fn = cls(desc.size, desc.domain, log=desc.log, safe_eval=desc.safe_eval)
    assert fn._linear_scale == desc.scale and fn._linear_shift == desc.shift and tuple(fn.ref_domain) == desc.ref_domain
    return fn


def _boot_device(case):
    """-> n [B, L, G], s, sp [B, L, G, C]: (G, C) = (1, M * R) shared, (M, K) per component"""
    import torch
    from mlmc_amd import engine
    if case.layout == "shared":
        fns = _fn(case.descs[0])
        acc = engine.BootstrapAccumulator(fns, case.M, case.L, case.B)
    else:
        fns = [_fn(d) for d in case.descs]
        acc = engine.ComponentBootstrapAccumulator(fns, case.K, case.L, case.B)
    for level, f, c, sizes, stream in case.calls:
        acc.accum(level, torch.from_numpy(f).cuda(), None if c is None else torch.from_numpy(np.ascontiguousarray(c)).cuda(), sizes,
                  case.seed, stream)
    n, s, sp = acc.finalize()
    acc.close()
    G, C = (1, case.M * case.K) if case.layout == "shared" else (case.M, case.K)
    return n.reshape(case.B, case.L, G), s.reshape(case.B, case.L, G, C), sp.reshape(case.B, case.L, G, C)


def _boot_weights(case):
    """The device's own exported weights: the kept counts [B, L, G] of EVERY replicate (from blocks of at most WEIGHT_BLOCK
    weights), the picks that fell on dropped samples, and per accum call the weight rows of the checked replicates, each taken
    on its own with b0 = b -- the same bits as its row of the block."""
    from mlmc_amd import engine
    G = 1 if case.layout == "shared" else case.M
    counts = np.zeros((case.B, case.L, G), dtype=np.int64)
    on_dropped, checked = 0, []
    for call in case.calls:
        level, f, _, sizes, stream = call
        n = f.shape[1]
        keep = gc.boot_keeps(case, call).astype(np.int64)                         # [G, n]
        nb = max(1, min(case.B, WEIGHT_BLOCK // n))
        rows = {}
        for b0 in range(0, case.B, nb):
            w = engine.bootstrap_weights(n, sizes[b0:b0 + nb], case.seed, stream, b0=b0).astype(np.int64)
            assert np.array_equal(w.sum(axis=1), sizes[b0:b0 + nb]) and w.min() >= 0
            kept = w @ keep.T
            counts[b0:b0 + nb, level, :] += kept
            on_dropped += int((sizes[b0:b0 + nb, None] - kept).sum())
            for b in case.checked:
                if b0 <= b < b0 + nb:
                    rows[b] = w[b - b0]
        one_by_one = []
        for b in case.checked:
            w = engine.bootstrap_weights(n, sizes[b:b + 1], case.seed, stream, b0=b)[0].astype(np.int64)
            assert np.array_equal(w, rows[b]), (case, level, b)
            one_by_one.append(w)
        checked.append(np.stack(one_by_one))
    return counts, on_dropped, checked


@pytest.mark.parametrize("name", list(gc.boot_cases()))
def test_bootstrap_sums_against_the_long_double_reference(hip, name):
    """One case of either layout: the kept counts of EVERY replicate are the exact integers sum w keep (per component in the
    per-component layout, where they ride through the MFMAs as a flag column), and s, sp of the checked replicates (0, 15, 16,
    63, 64, 256, B - 1) sit within the class tolerance of the long-double weighted sums under the device's exported weights."""
    case = gc.boot_cases()[name]
    n, s, sp = _boot_device(case)
    counts, on_dropped, weights = _boot_weights(case)
    assert np.array_equal(n, counts), (case, np.argwhere(n != counts)[:8].tolist())
    assert on_dropped > 0, case                                                # dropped samples did carry positive weights
    rn, rs, rsp, S, SP = gc.boot_sums(case, weights)
    assert np.array_equal(rn, counts[case.checked])
    worst = Worst()
    for q, got, want, scale in (("s", s[case.checked], rs, S), ("sp", sp[case.checked], rsp, SP)):
        units, flat = ax.worst(got, want, scale)
        k, level, g, col = np.unravel_index(flat, want.shape)
        R = case.K
        place = "{} replicate {} level {} component {} term {}".format(
            case.name, case.checked[k], level, col // R if case.layout == "shared" else g, col % R)
        worst.add("{} {}".format(case.cls, q), units, gc.boot_tolerance(case.cls, q), place)
    worst.show(name)
    assert not worst.failures, worst.failures[:8]
