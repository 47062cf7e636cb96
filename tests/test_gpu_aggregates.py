"""GPU tests of mlmc_scenario_aggregates and mlmc_rows_weighted_sums through the C ABI: the first bit for bit against the NumPy
reference of tests/aggregate_cases.py (itself checked against exact chains in tests/test_aggregates_cpu.py), the second with exact
counts and sums within the gate that the fp64 twin of the kernel's order fixed there."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import aggregate_cases as ac

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 4097)
PAD_IN, PAD_OUT = 7.0e77, -3.0e33          # what lies beyond the columns: never read into a result, never overwritten


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


def _aggregates(hip, x, W, members, lower, upper, extras, kind):
    """mlmc_scenario_aggregates on x [S, M, n] with ld = n + 3 and ld_out = n + 1 -> agg [S, Q, n]; the padding must come back untouched"""
    import torch
    S, M, n = x.shape
    A = 0 if W is None else W.shape[0]
    Q = A + bin(extras).count("1")
    ld, ld_out = n + 3, n + 1
    xp = np.full((S, M, ld), PAD_IN)
    xp[:, :, :n] = x
    out = np.full((S, Q, ld_out), PAD_OUT)
    if kind == hip.DEVICE:
        xp, out = torch.from_numpy(xp).cuda(), torch.from_numpy(out).cuda()
        torch.cuda.synchronize()
    hip.check(hip.lib().mlmc_scenario_aggregates(hip.ptr(xp), S, M, n, ld, hip.ptr(W), A, hip.ptr(members), hip.ptr(lower), hip.ptr(upper),
                                                 extras, hip.ptr(out), ld_out, kind))
    out = out.cpu().numpy() if kind == hip.DEVICE else out
    assert np.all(out[:, :, n:] == PAD_OUT)
    return np.ascontiguousarray(out[:, :, :n])


def _check(got, x, W, members, lower, upper, extras, tag):
    """bit for bit the reference; the ARGMAX / ARGMIN rows as integers, MAX / MIN as x at that index"""
    ref = ac.aggregates_reference(x, W, members, lower, upper, extras)
    assert got.shape == ref.shape, tag
    assert ac.same_bits(got, ref), (tag, np.argwhere(got.view(np.uint64) != ref.view(np.uint64))[:4].tolist())
    A = 0 if W is None else W.shape[0]
    names = [name for name, bit in zip(("max", "min", "count", "argmax", "argmin"), ac.EXTRA_BITS) if extras & bit]
    S, M, n = x.shape
    for arg, val in (("argmax", "max"), ("argmin", "min")):
        if arg in names and n:
            idx = got[:, A + names.index(arg), :].astype(np.int64)
            assert np.array_equal(idx, got[:, A + names.index(arg), :]) and idx.min() >= 0 and idx.max() < M, tag
            if val in names:
                at = np.take_along_axis(x, idx[:, None, :], axis=1)[:, 0, :]
                assert ac.same_bits(got[:, A + names.index(val), :], at), tag


@pytest.mark.parametrize("M", [1, 2, 5, 64, 65, 130])
def test_aggregates_bit_for_bit(hip, M):
    """every size, number of linear rows and of sets, host and device memory; the extra rows, members and limits rotate through their
    combinations (every subset of the extras occurs for every M)"""
    subsets = itertools.cycle(range(32))
    kinds = itertools.cycle(itertools.product(("all", "one", "alternating"), ("finite", "one-sided")))
    seen = set()
    for n in SIZES:
        for A in (0, 1, 3, 17):
            for S in (1, 3):
                x = ac.scenario_inputs(S, M, n, seed=1000 * M + n)
                W = ac.scenario_weights(A, M, seed=A)
                extras = next(subsets)
                mk, lk = next(kinds)
                members = ac.scenario_members(mk, M)
                lower, upper = ac.scenario_limits(lk, M)
                if lk == "one-sided" and (M + n) % 2:
                    upper = None                                   # a NULL side is no limit on that side
                seen.add(extras)
                for kind in (hip.HOST, hip.DEVICE):
                    got = _aggregates(hip, x, W, members, lower, upper, extras, kind)
                    _check(got, x, W, members, lower, upper, extras, (M, n, A, S, extras, mk, lk, kind))
    assert seen == set(range(32))


def test_aggregates_every_subset_members_and_limits(hip):
    """one shape with several blocks, every subset of the extras x every kind of members x every kind of limits (without limits the
    count row is an error of the call)"""
    S, M, n = 2, 5, 257
    x = ac.scenario_inputs(S, M, n, seed=8)
    W = ac.scenario_weights(3, M, seed=9)
    for extras in range(32):
        for mk in ("all", "one", "alternating"):
            for lk in ("finite", "one-sided", "none"):
                members = ac.scenario_members(mk, M)
                lower, upper = ac.scenario_limits(lk, M)
                if lk == "none" and extras & ac.AGG_COUNT:
                    with pytest.raises(hip.MlmcHipError, match="without limits"):
                        _aggregates(hip, x, W, members, None, None, extras, hip.DEVICE)
                    continue
                got = _aggregates(hip, x, W, members, lower, upper, extras, hip.DEVICE)
                _check(got, x, W, members, lower, upper, extras, (extras, mk, lk))


def test_aggregates_do_not_depend_on_sets_or_blocks(hip):
    """a set alone and inside S = 3; columns [50, 150) of a call and a call on that slice; a NaN in a non-member is not seen"""
    M, n = 65, 257
    x = ac.scenario_inputs(3, M, n, seed=21)
    W = ac.scenario_weights(17, M, seed=22)
    members = ac.scenario_members("alternating", M)
    lower, upper = ac.scenario_limits("finite", M)
    every = 31
    full = _aggregates(hip, x, W, members, lower, upper, every, hip.DEVICE)
    for s in range(3):
        alone = _aggregates(hip, x[s:s + 1], W, members, lower, upper, every, hip.DEVICE)
        assert ac.same_bits(alone[0], full[s]), s
    part = _aggregates(hip, np.ascontiguousarray(x[:, :, 50:150]), W, members, lower, upper, every, hip.HOST)
    assert ac.same_bits(part, full[:, :, 50:150])
    j = (7 * 1 + 3) % n                                      # component 0 holds a NaN there and is no member
    assert np.isnan(x[0, 0, j]) and not members[0] and not np.isnan(full[0, 17, j])


def test_unit_weight_reproduces_its_row(hip):
    """W = e_m gives row m under == where the other components are finite; +0 + (-0) = +0 is the one allowed difference in bits: a
    -0.0 of the row comes back as +0.0"""
    M, n = 5, 300
    x = np.random.default_rng(31).standard_normal((1, M, n))
    x[0, 2, 10] = -0.0
    x[0, 2, 11] = np.nan
    x[0, 2, 12] = np.inf
    for m in range(M):
        e = np.zeros((1, M))
        e[0, m] = 1.0
        got = _aggregates(hip, x, e, None, None, None, 0, hip.DEVICE)[0, 0]
        if m == 2:
            assert np.array_equal(got, x[0, m], equal_nan=True)
            diff = np.flatnonzero(got.view(np.uint64) != x[0, m].view(np.uint64))
            assert diff.tolist() == [10] and got[10] == 0.0 and not np.signbit(got[10])
        else:
            fin = np.ones(n, dtype=bool)
            fin[[11, 12]] = False                            # 0 * NaN and 0 * inf of component 2
            assert ac.same_bits(got[fin], x[0, m][fin]) and np.isnan(got[~fin]).all()


def test_aggregates_argument_errors(hip):
    x = np.zeros((1, 3, 8))
    call = lambda **kw: _aggregates(hip, x, kw.get("W"), kw.get("members"), kw.get("lower"), kw.get("upper"), kw.get("extras", 0),
                                    hip.HOST)
    with pytest.raises(hip.MlmcHipError, match="no component is a member"):
        call(extras=ac.AGG_MAX, members=np.zeros(3, dtype=np.uint8))
    with pytest.raises(hip.MlmcHipError, match="limit of component 1 is NaN"):
        call(extras=ac.AGG_COUNT, lower=np.array([0.0, np.nan, 0.0]))
    with pytest.raises(hip.MlmcHipError, match="row 0, component 2 is not finite"):
        call(W=np.array([[1.0, 2.0, np.inf]]))
    with pytest.raises(hip.MlmcHipError, match="unknown bits"):
        call(extras=64)
    lib = hip.lib()
    out = np.zeros((1, 1, 8))
    W = np.ones((1, 3))
    assert lib.mlmc_scenario_aggregates(hip.ptr(x), 1, 3, 8, 7, hip.ptr(W), 1, None, None, None, 0, hip.ptr(out), 8, hip.HOST) != 0
    assert lib.mlmc_scenario_aggregates(hip.ptr(x), 1, 3, 8, 8, hip.ptr(W), 1, None, None, None, 0, hip.ptr(out), 7, hip.HOST) != 0
    assert lib.mlmc_scenario_aggregates(hip.ptr(x), 0, 3, 8, 8, hip.ptr(W), 1, None, None, None, 0, hip.ptr(out), 8, hip.HOST) != 0
    assert lib.mlmc_scenario_aggregates(hip.ptr(x), 1, 3, 8, 8, hip.ptr(W), 1, None, None, None, 0, hip.ptr(out), 8, 5) != 0
    assert lib.mlmc_scenario_aggregates(None, 1, 3, 8, 8, hip.ptr(W), 1, None, None, None, 0, hip.ptr(out), 8, hip.HOST) != 0


# ---- mlmc_rows_weighted_sums --------------------------------------------------------------------------------------------------
def _sums(hip, y, f, c, t, lower, kind, pad=3):
    """y [Rw, n] (ld = n + pad), f [n] or None, c [Rw] or None, t [Rw, P] -> (n_used, n_skipped, sums [Rw, 3], tails [Rw, P, 2])"""
    import torch
    Rw, n = y.shape
    P = t.shape[1]
    yp = np.full((Rw, n + pad), np.nan)
    yp[:, :n] = y
    fp = None if f is None else np.ascontiguousarray(f, dtype=np.float64)
    if kind == hip.DEVICE:
        yp = torch.from_numpy(yp).cuda()
        fp = None if fp is None else torch.from_numpy(fp).cuda()
        torch.cuda.synchronize()
    used, skipped = np.full(Rw, -1, dtype=np.int64), np.full(Rw, -1, dtype=np.int64)
    sums, tails = np.full((Rw, 3), np.nan), np.full((Rw, P, 2), np.nan)
    t = np.ascontiguousarray(t, dtype=np.float64)
    hip.check(hip.lib().mlmc_rows_weighted_sums(hip.ptr(yp), Rw, n, n + pad, hip.ptr(fp), hip.ptr(c), hip.ptr(t), P,
                                                1 if lower else 0, hip.ptr(used), hip.ptr(skipped), hip.ptr(sums), hip.ptr(tails), kind))
    return used, skipped, sums, tails


def test_weighted_sums_within_the_gate(hip):
    """the cases the twin was measured on (tests/aggregate_cases.py), each as a row of its own: counts exact, sums within the gate;
    prints the device's own worst distance"""
    worst_first = worst_second = 0.0
    for name, y, f, c, t in ac.sum_cases():
        used, skipped, sums, tails = _sums(hip, y[None, :], f, np.array([c]), t[None, :], False, hip.DEVICE)
        used_r, ref = ac.weighted_sums_ld(y, f, c, t)
        assert used[0] == used_r and skipped[0] == y.size - used_r, name
        got = np.concatenate([sums[0], tails[0].reshape(-1)])
        first, second = ac.distances(got, ref, ac.sum_units(y, f, c))
        worst_first, worst_second = max(worst_first, first), max(worst_second, second)
        assert first <= ac.GATE_FIRST and second <= ac.GATE_SECOND, (name, first, second)
    print("device worst: first sums {:.3f} (gate {}), second sums {:.3f} (gate {}) units".format(
        worst_first, ac.GATE_FIRST, worst_second, ac.GATE_SECOND))


@pytest.mark.parametrize("Rw", [1, 3, 17])
def test_weighted_sums_rows(hip, Rw):
    """Rw rows at every size (and 20011), weights NULL / random / with exact zeros, NaN in y and in f, both tails, host and device:
    counts exact -- with f NULL the tail sums ARE counts, so the >= / <= edge at a data value is exact -- sums within the gate, two
    calls and both memory kinds give identical bits"""
    for i, n in enumerate(SIZES + (20011,)):
        rng = np.random.default_rng(50 * Rw + i)
        y = np.stack([ac.sum_row("offset" if r % 2 else "lognormal", n, 7 * r + i) for r in range(Rw)]) if n else np.zeros((Rw, 0))
        if n > 3:
            y[0, n // 2] = np.nan
            y[Rw - 1, 1] = np.nan
        for wk in (None, "random", "zeros"):
            f = ac.sum_weights(wk, n, i) if n else (None if wk is None else np.zeros(0))
            if f is not None and n > 3:
                f[2] = np.nan
            t = np.stack([ac.row_thresholds(y[r]) for r in range(Rw)]) if n else np.zeros((Rw, 4))
            c = np.array([0.0 if r % 3 == 0 else float(np.nanmean(y[r])) for r in range(Rw)]) if n else np.zeros(Rw)
            for lower in (False, True):
                got = _sums(hip, y, f, c, t, lower, hip.DEVICE)
                again = _sums(hip, y, f, c, t, lower, hip.DEVICE)
                host = _sums(hip, y, f, c, t, lower, hip.HOST, pad=1)
                for a, b, h in zip(got, again, host):
                    assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b)
                    assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, h.view(np.uint64) if h.dtype == np.float64 else h)
                used, skipped, sums, tails = got
                if n == 0:
                    assert not used.any() and not skipped.any() and not sums.any() and not tails.any()
                    continue
                for r in range(Rw):
                    used_r, ref = ac.weighted_sums_ld(y[r], f, c[r], t[r], lower)
                    assert used[r] == used_r and skipped[r] == n - used_r, (n, wk, r)
                    flat = np.concatenate([sums[r], tails[r].reshape(-1)])
                    first, second = ac.distances(flat, ref, ac.sum_units(y[r], f, c[r]))
                    assert first <= ac.GATE_FIRST and second <= ac.GATE_SECOND, (n, wk, lower, r, first, second)
                    if f is None:
                        with np.errstate(invalid="ignore"):
                            counts = [np.sum((y[r] <= tk) if lower else (y[r] >= tk)) for tk in t[r]]
                        assert tails[r, :, 0].tolist() == counts, (n, lower, r)


def test_weighted_sums_row_alone_and_among_17(hip):
    """a row's bits depend on its own data and n alone: not on the other rows, its position or the number of thresholds around it"""
    n, Rw = 20011, 17
    y = np.stack([ac.sum_row("lognormal", n, 300 + r) for r in range(Rw)])
    f = ac.sum_weights("zeros", n, 5)
    t = np.stack([np.quantile(y[r], np.linspace(0.05, 0.95, 11)) for r in range(Rw)])       # 11 thresholds: two passes
    c = y.mean(axis=1)
    full = _sums(hip, y, f, c, t, False, hip.DEVICE)
    for r in (0, 8, 16):
        alone = _sums(hip, y[r:r + 1], f, c[r:r + 1], t[r:r + 1], False, hip.DEVICE)
        for a, b in zip(alone, full):
            assert np.array_equal(a[0], b[r]), r
        first3 = _sums(hip, y[r:r + 1], f, c[r:r + 1], t[r:r + 1, :3], False, hip.DEVICE)
        assert np.array_equal(first3[2][0], full[2][r]) and np.array_equal(first3[3][0], full[3][r][:3])
    ref_used, ref = ac.weighted_sums_ld(y[3], f, c[3], t[3])
    flat = np.concatenate([full[2][3], full[3][3].reshape(-1)])
    first, second = ac.distances(flat, ref, ac.sum_units(y[3], f, c[3]))
    assert first <= ac.GATE_FIRST and second <= ac.GATE_SECOND


def test_weighted_sums_errors(hip):
    y = np.random.default_rng(1).standard_normal((2, 100))
    t = np.zeros((2, 1))
    for bad in (-1e-3, np.inf):
        f = np.ones(100)
        f[37] = bad
        for kind in (hip.HOST, hip.DEVICE):
            with pytest.raises(hip.MlmcHipError, match="negative or infinite"):
                _sums(hip, y, f, None, t, False, kind)
    f = np.ones(100)
    f[37] = -1.0
    y2 = y.copy()
    y2[:, 37] = np.nan                                        # a skipped column: its weight is not looked at
    used, skipped, _, _ = _sums(hip, y2, f, None, t, False, hip.DEVICE)
    assert used.tolist() == [99, 99] and skipped.tolist() == [1, 1]
    with pytest.raises(hip.MlmcHipError, match="threshold of row 1 is NaN"):
        _sums(hip, y, None, None, np.array([[0.0], [np.nan]]), False, hip.HOST)
    with pytest.raises(hip.MlmcHipError, match="centre of row 0 is not finite"):
        _sums(hip, y, None, np.array([np.inf, 0.0]), t, False, hip.HOST)
    lib = hip.lib()
    u, s, sums = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64), np.zeros((2, 3))
    args = lambda ld, tail, kind: (hip.ptr(y), 2, 100, ld, None, None, None, 0, tail, hip.ptr(u), hip.ptr(s), hip.ptr(sums), None, kind)
    assert lib.mlmc_rows_weighted_sums(*args(99, 0, hip.HOST)) != 0
    assert lib.mlmc_rows_weighted_sums(*args(100, 2, hip.HOST)) != 0
    assert lib.mlmc_rows_weighted_sums(*args(100, 0, 7)) != 0
    assert lib.mlmc_rows_weighted_sums(*args(100, 0, hip.HOST)) == 0 and u.tolist() == [100, 100]
