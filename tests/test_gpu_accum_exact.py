"""GPU checks of the sample-accumulation kernels (k_moments_accum, k_moments_accum_split, k_spline_accum, k_moments_multi_var,
k_cov_accum*) and of the evaluation-only kernel (k_eval) against the 80-bit long-double reference of tests/accum_exact.py, in
units of 2^-53 * (first-order condition scale).  The cases and tolerances are those of tests/accum_cases.py: the tolerance of a
class is max(16, 4 x the worse of the two fp64 twins), calibrated without a device by tests/test_accum_exact_cpu.py.  Every
test prints its worst units with the case, level and term where they occur (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

from tests import accum_cases as ac
from tests import accum_exact as ax

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


def _fn(desc):
    from mlmc_amd import Fourier, Legendre, Monomial, Spline
    cls = {ax.LEGENDRE: Legendre, ax.MONOMIAL: Monomial, ax.FOURIER: Fourier, ax.SPLINE: Spline}[desc.kind]
    fn = cls(desc.size, desc.domain, log=desc.log, safe_eval=desc.safe_eval)
    assert fn._linear_scale == desc.scale and fn._linear_shift == desc.shift and tuple(fn.ref_domain) == desc.ref_domain
    return fn


def _accumulator(case):
    from mlmc_amd.engine import LevelAccumulator
    mode = LevelAccumulator.COV if case.entry == "cov" else LevelAccumulator.MOMENTS
    return LevelAccumulator(_fn(case.desc), case.L, mode, n_comp=case.M, mean_only=(case.entry == "mean_only"))


def _host(case):
    """one push per level from host arrays, then finalize"""
    acc = _accumulator(case)
    for l, (f, c) in enumerate(case.levels):
        if case.M == 1:
            acc.push(l, f[0], None if c is None else c[0])
        else:
            acc.push(l, f, c)
    out = acc.finalize()
    acc.close()
    return out


def _device_chunks(case):
    import torch
    chunks = []
    for l, (f, c) in enumerate(case.levels):
        if case.M == 1 and case.entry != "component":
            f, c = f[0], None if c is None else c[0]
        chunks.append((l, torch.from_numpy(np.ascontiguousarray(f)).cuda(), None if c is None else torch.from_numpy(np.ascontiguousarray(c)).cuda()))
    torch.cuda.synchronize()
    return chunks


def _device(case):
    """all levels from device-resident tensors in one launch (mlmc_accum_estimate)"""
    acc = _accumulator(case)
    out = acc.estimate(_device_chunks(case))
    acc.close()
    return out


def _component_entries(hip, case, chunks):
    """mlmc_accum_estimate_multi (means only) and mlmc_accum_estimate_multi_var on the device chunks -> (n, n_rm, s), (n, n_rm, s, sp)
    with n [L, M], s [L, M, K]"""
    lib, M, L, K = hip.lib(), case.M, case.L, case.desc.size
    fns = [_fn(d) for d in case.descs]
    arr = (C.c_void_p * M)(*[fn._basis_handle().value for fn in fns])
    lv = np.array([c[0] for c in chunks], dtype=np.int32)
    nn = np.array([c[1].shape[1] for c in chunks], dtype=np.int64)
    fp = (C.c_void_p * len(chunks))(*[c[1].data_ptr() for c in chunks])
    cp = (C.c_void_p * len(chunks))(*[None if c[2] is None else c[2].data_ptr() for c in chunks])
    out = []
    for entry, n_float in ((lib.mlmc_accum_estimate_multi, 1), (lib.mlmc_accum_estimate_multi_var, 2)):
        n, n_rm = np.zeros((L, M), dtype=np.int64), np.zeros((L, M), dtype=np.int64)
        sums = [np.zeros((L, M, K)) for _ in range(n_float)]
        hip.check(entry(M, C.cast(arr, C.c_void_p), K, L, len(chunks), hip.ptr(lv), C.cast(fp, C.c_void_p), C.cast(cp, C.c_void_p),
                        hip.ptr(nn), hip.ptr(n), hip.ptr(n_rm), *[hip.ptr(v) for v in sums]))
        out.append((n, n_rm, *sums))
    return out


def _where(case, shape, flat):
    idx = np.unravel_index(flat, shape)
    if case.entry == "component":
        return "level {} component {} term {}".format(*idx)
    R = case.desc.size
    if case.entry == "cov":
        return "level {} entry ({}, {})".format(idx[0], idx[1] // R, idx[1] % R)
    return "level {}{} term {}".format(idx[0], " component {}".format(idx[1] // R) if case.M > 1 else "", idx[1] % R)


class Worst:
    """the worst units of a test per quantity, with the place; the entries over their tolerance (a test prints all its figures
    before it fails)"""

    def __init__(self):
        self.w = {}
        self.failures = []

    def check(self, ok, *what):
        if not ok:
            self.failures.append(what)

    def add(self, q, units, place):
        if q not in self.w or units > self.w[q][0]:
            self.w[q] = (units, place)

    def show(self, title):
        for q, (units, place) in sorted(self.w.items()):
            print("{:28s} {:6s} worst {:10.4g} units  at {}".format(title, q, units, place))


def _judge(case, got, label, worst):
    """counts exactly, every entry of every judged quantity within the class tolerance of the long-double reference, exact zeros
    where every kept difference is zero, NaN where the mean-only entry documents it"""
    ref = ac.reference(case)
    n, n_rm, s = got[0], got[1], got[2]
    sp = got[3] if len(got) > 3 else None
    assert np.array_equal(n, ref.n) and np.array_equal(n_rm, ref.n_rm), (case, label, n, ref.n, n_rm, ref.n_rm)
    s = np.asarray(s).reshape(ref.s.shape)
    # the constant sums to the count, exactly: row 0 of every component on level 0 (a covariance: entry (0, 0))
    if case.entry == "component":
        assert np.array_equal(s[0, :, 0], n[0].astype(np.float64)), (case, label)
    else:
        first = s[0].reshape(case.M, -1)[:, 0]
        assert np.array_equal(first, np.full(case.M, float(n[0]))), (case, label, first, n[0])
    if case.entry == "mean_only":
        assert sp is not None and np.all(np.isnan(sp)), (case, label)
    values = {"cov_s" if case.entry == "cov" else "s": s}
    if sp is not None and case.entry not in ("mean_only", "cov"):
        values["sp"] = np.asarray(sp).reshape(ref.sp.shape)
    for q in ac.quantities(case):
        if q not in values:
            continue                                                                    # the means-only component entry has no sp
        want, scale = ac.judged(ref, q)
        units, flat = ax.worst(values[q], want, scale)
        place = "{} [{}] {}".format(case.name, label, _where(case, want.shape, flat))
        worst.add(q, units, place)
        worst.check(units <= ac.tolerance(case.cls, q), q, units, ac.tolerance(case.cls, q), place)
    if ref.SP is not None:
        zero = np.asarray(ref.SP == 0)              # d = 0 in every kept sample (row 0 of a pair level, fine == coarse, no support)
        worst.check(np.all(s[zero] == 0), "exact zeros of s", case, label, np.argwhere(zero & (s != 0))[:4].tolist())
        if "sp" in values:
            worst.check(np.all(values["sp"][zero] == 0), "exact zeros of sp", case, label)
    return values


def _agree(case, a, b, label, worst):
    """two routes of the same sums (another grid split may add in another order): within the class tolerance of each other"""
    ref = ac.reference(case)
    for q in a:
        _, scale = ac.judged(ref, q)
        units, flat = ax.worst(a[q], b[q], scale)
        worst.add(q + " " + label, units, "{} {}".format(case.name, _where(case, scale.shape, flat)))
        worst.check(units <= ac.tolerance(case.cls, q), case, label, q, units, ac.tolerance(case.cls, q))


def _same_bits(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


GROUPS = {}
for _case in ac.cases().values():
    GROUPS.setdefault("{}-{}".format(_case.entry, _case.cls), []).append(_case)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_level_sums_against_the_long_double_reference(hip, group):
    """Every case of one entry and tolerance class: counts, every sum in units of its condition scale, exact zeros, NaN where
    documented; a second call gives the same bits; device-resident inputs (all levels in one launch) against the reference and
    against the host route.  The per-component cases run both C entries on the same device chunks."""
    worst = Worst()
    for case in GROUPS[group]:
        if case.entry == "component":
            chunks = _device_chunks(case)
            (n0, rm0, sums), var = _component_entries(hip, case, chunks)
            again = _component_entries(hip, case, chunks)
            assert _same_bits((n0, rm0, sums), again[0]) and _same_bits(var, again[1]), case
            _judge(case, (n0, rm0, sums), "multi", worst)
            _judge(case, var, "multi_var", worst)
            continue
        got = _host(case)
        assert _same_bits(got, _host(case)), case                                   # a second call returns the same bits
        values = _judge(case, got, "host", worst)
        if case.device:
            dev = _device(case)
            assert _same_bits(dev, _device(case)), case
            _agree(case, values, _judge(case, dev, "device", worst), "host/device", worst)
    print()
    worst.show(group)
    assert not worst.failures, worst.failures[:8]


@pytest.mark.parametrize("name", sorted(ac.EVAL_CASES))
def test_eval_all_against_the_long_double_rows(hip, name):
    """Moments.eval_all (k_eval) at the hand-placed values and a 1501-point grid: every value within 4 x the worse fp64 twin of
    the long-double row, unit 2^-53 max(|value|, 1); dropped values give NaN rows (Fourier keeps its constant column)."""
    desc, x = ac.eval_desc(name), ac.eval_points(name)
    got = _fn(desc).eval_all(x)
    ref, keep = ax.eval_rows(desc, x)
    assert got.shape == ref.shape and keep.sum() > 1500 and (~keep).sum() >= 2
    first = 1 if desc.kind == ax.FOURIER else 0
    assert np.all(np.isnan(got[~keep][:, first:])) and np.all(got[~keep][:, :first] == 1)
    units, flat = ax.worst(got[keep], ref[keep], np.maximum(np.abs(ref[keep]), 1))
    i, k = np.unravel_index(flat, ref[keep].shape)
    print("\n{:28s} worst {:10.4g} units  at x = {!r} term {}  (tolerance {:.4g})".format(name, units, float(x[keep][i]), k, ac.eval_tolerance(name)))
    assert units <= ac.eval_tolerance(name), (name, units, float(x[keep][i]), k)
    assert np.array_equal(got, _fn(desc).eval_all(x), equal_nan=True)
