"""GPU tests of mlmc_concordance_counts (mlmc_amd/csrc/concordance.hip) through tool.simple_distribution.concordance_counts and
the raw entry: every counter equals the NumPy twin of tests/concordance_cases.py integer for integer -- the counts are integers,
so there is no tolerance anywhere in this file."""
import numpy as np
import pytest

from tests import concordance_cases as cc

pytestmark = pytest.mark.gpu
M_SET = (1, 2, 3, 17, 65)
N_SET = (0, 1, 63, 64, 65, 127, 129, 1000)
INF = np.inf


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


def _values(rng, M, n, coarse, nan=True):
    """half-integers in [-1.5, 1.5] (many sit exactly on the limits of _events), a few +-inf, and with `nan` a NaN in about one
    column in eight, in single rows of fine or of coarse"""
    f = rng.integers(-3, 4, size=(M, n)) * 0.5
    c = f + rng.integers(-1, 2, size=(M, n)) * 0.5 if coarse else None
    for x in (f, c):
        if x is None or n == 0:
            continue
        x[rng.integers(0, M, size=max(1, n // 50)), rng.integers(0, n, size=max(1, n // 50))] = INF
        x[rng.integers(0, M, size=max(1, n // 50)), rng.integers(0, n, size=max(1, n // 50))] = -INF
        if nan:
            k = max(1, n // 16)
            x[rng.integers(0, M, size=k), rng.integers(0, n, size=k)] = np.nan
    return f, c


def _events(rng, M, G):
    lower = np.stack([np.full(M, -1.0), np.full(M, -INF), rng.integers(-2, 1, size=M) * 0.5])
    upper = np.stack([np.full(M, 1.0), np.full(M, INF), np.where(rng.integers(0, 2, size=M) == 0, INF, 1.0)])
    return lower[:G].copy(), upper[:G].copy()


def _padded(x, pad):
    """x [M, n] as a device view with the row stride n + pad; the padding holds NaN"""
    import torch
    if x is None:
        return None
    buf = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :x.shape[1]] = torch.from_numpy(x)
    return buf[:, :x.shape[1]]


def _equal(got, ref):
    pair, all_, kept = ref
    assert got.pair.dtype == np.int64 and got.all.dtype == np.int64 and got.kept.dtype == np.int64
    assert np.array_equal(got.pair, pair), np.argwhere(got.pair != pair)[:5]
    assert np.array_equal(got.all, all_), (got.all, all_)
    assert got.kept.shape == (1,) and int(got.kept[0]) == int(kept)


@pytest.mark.parametrize("M", M_SET)
def test_counts_equal_the_twin(hip, M):
    from mlmc_amd.tool import simple_distribution as sd
    rng = np.random.default_rng(100 + M)
    for n in N_SET:
        for coarse in (False, True):
            f, c = _values(rng, M, n, coarse)
            for G in (1, 3):
                lower, upper = _events(rng, M, G)
                ref = cc.twin_counts(f, c, lower, upper)
                _equal(sd.concordance_counts(f, c, lower, upper), ref)                                   # ld = n
                _equal(sd.concordance_counts(_padded(f, 3), _padded(c, 3), lower, upper), ref)           # ld = n + 3
            if n == 1000:
                assert 0 < ref[2] < n and ref[0][0, 0].max() > 0


def test_across_pair_tiles_word_groups_and_runs(hip):
    """M = 130 is four pair tiles of 32 rows and two rows of a fifth (CG_TILE); n = 4097 is 65 words: two staging groups of 32
    words and one word of a third (CG_WORDS), which the 45 (tile pair, event) workgroups of G = 3 walk in runs of 32 words, so a
    counter takes the atomics of three workgroups"""
    from mlmc_amd.tool import simple_distribution as sd
    rng = np.random.default_rng(7)
    M, n = 130, 4097
    f, c = _values(rng, M, n, True, nan=False)
    f[5, 4096] = np.nan                                              # the one column of the last word
    c[129, 64] = np.nan
    lower, upper = _events(rng, M, 3)
    ref = cc.twin_counts(f, c, lower, upper)
    assert ref[2] == n - 2
    _equal(sd.concordance_counts(f, c, lower, upper), ref)
    _equal(sd.concordance_counts(f, None, lower, upper), cc.twin_counts(f, None, lower, upper))


def test_slabs_of_columns_change_nothing(hip, monkeypatch):
    """the entry walks the columns in slabs that bound its bit matrix; MLMC_CONCORDANCE_SLAB_WORDS = 32 makes n = 4097 three slabs
    (32 + 32 + 1 words), each with its own launches into the same counters"""
    from mlmc_amd.tool import simple_distribution as sd
    rng = np.random.default_rng(70)
    M, n = 5, 4097
    f, c = _values(rng, M, n, True)
    lower, upper = _events(rng, M, 3)
    ref = cc.twin_counts(f, c, lower, upper)
    one = sd.concordance_counts(f, c, lower, upper)
    monkeypatch.setenv("MLMC_CONCORDANCE_SLAB_WORDS", "32")
    _equal(sd.concordance_counts(f, c, lower, upper), ref)
    _equal(sd.concordance_counts(_padded(f, 3), _padded(c, 3), lower, upper), ref)
    _equal(sd.concordance_counts(f, None, lower, upper), cc.twin_counts(f, None, lower, upper))
    few = sd.concordance_counts(f, c, lower, upper, pairs=False)
    assert few.pair is None and np.array_equal(few.all, ref[1]) and few.kept[0] == ref[2]
    assert all(np.array_equal(a, b) for a, b in zip(one, sd.concordance_counts(f, c, lower, upper)))


def test_limits_nans_and_infinities(hip):
    from mlmc_amd.tool import simple_distribution as sd
    rng = np.random.default_rng(8)
    M, n = 3, 200
    f, c = _values(rng, M, n, True, nan=False)
    # limits of +-inf: every finite value is inside, an infinite one is not (the box is open)
    got = sd.concordance_counts(f, c, np.full(M, -INF), np.full(M, INF))
    _equal(got, cc.twin_counts(f, c, np.full(M, -INF), np.full(M, INF)))
    assert got.kept[0] == n and got.pair[0, 0, 0, 0] == np.count_nonzero(np.isfinite(f[0]))
    # values exactly on a limit are outside
    on = np.tile(np.array([0.5, 1.0, 0.5, 0.0]), (M, 50))
    got = sd.concordance_counts(on, None, np.full(M, 0.5), np.full(M, 1.0))
    assert np.all(got.pair == 0) and np.all(got.all == 0) and got.kept[0] == 200
    got = sd.concordance_counts(on, None, np.full(M, 0.0), np.full(M, 1.0))
    assert np.all(got.pair[0, 0] == 100) and got.all[0, 0] == 100
    # NaN in single rows of fine only, of coarse only, in the last partial word, in every column
    for where in ("fine", "coarse", "last word", "every column"):
        f2, c2 = f.copy(), c.copy()
        if where == "fine":
            f2[1, 3::7] = np.nan
        elif where == "coarse":
            c2[2, 5::11] = np.nan
        elif where == "last word":
            f2[0, 192:] = np.nan                                     # columns 192 .. 199: the 8 columns of the fourth word
        else:
            f2[0, 0::2] = np.nan
            c2[2, 1::2] = np.nan
        lower, upper = _events(rng, M, 3)
        ref = cc.twin_counts(f2, c2, lower, upper)
        got = sd.concordance_counts(f2, c2, lower, upper)
        _equal(got, ref)
        if where == "every column":
            assert got.kept[0] == 0 and np.all(got.pair == 0) and np.all(got.all == 0)
        if where == "last word":
            assert got.kept[0] == 192
    # a dropped column contributes to nothing: the counts are those of the kept columns alone
    f2 = f.copy()
    f2[1, 3::7] = np.nan
    keep = ~np.isnan(f2).any(axis=0)
    lower, upper = _events(rng, M, 3)
    _equal(sd.concordance_counts(f2, c, lower, upper), cc.twin_counts(f[:, keep], c[:, keep], lower, upper))


def test_accumulation_repeatability_and_residency(hip):
    import torch
    from mlmc_amd.tool import simple_distribution as sd
    rng = np.random.default_rng(9)
    M, n = 17, 1000
    f, c = _values(rng, M, n, True)
    lower, upper = _events(rng, M, 3)
    whole = sd.concordance_counts(f, c, lower, upper)
    _equal(whole, cc.twin_counts(f, c, lower, upper))
    again = sd.concordance_counts(f, c, lower, upper)
    assert all(np.array_equal(a, b) for a, b in zip(whole, again))
    # two calls on the halves, split off a multiple of 64 and off no multiple: the counters of the second add to the first
    for cut in (448, 333):
        out = sd.concordance_counts(f[:, :cut], c[:, :cut], lower, upper, device=True)
        assert all(t.is_cuda and t.dtype == torch.int64 for t in out)
        back = sd.concordance_counts(f[:, cut:], c[:, cut:], lower, upper, out=out, device=True)
        assert all(a.data_ptr() == b.data_ptr() for a, b in zip(out, back))
        assert all(np.array_equal(t.cpu().numpy(), w) for t, w in zip(out, whole))
    # a second call adds to the first
    twice = sd.concordance_counts(f, c, lower, upper, out=sd.concordance_counts(f, c, lower, upper, device=True))
    assert all(np.array_equal(t, 2 * w) for t, w in zip(twice, whole))
    # device-resident inputs
    ft, ct = torch.from_numpy(f).cuda(), torch.from_numpy(c).cuda()
    resident = sd.concordance_counts(ft, ct, lower, upper)
    assert all(np.array_equal(a, b) for a, b in zip(whole, resident))
    # pairs=False: the `all` counters of the full call, no pair matrix
    few = sd.concordance_counts(ft, ct, lower, upper, pairs=False)
    assert few.pair is None and np.array_equal(few.all, whole.all) and np.array_equal(few.kept, whole.kept)
    few = sd.concordance_counts(f, None, lower, upper, pairs=False)
    ref = cc.twin_counts(f, None, lower, upper)
    assert np.array_equal(few.all, ref[1]) and few.kept[0] == ref[2]
    # the kernel times are reported when asked for
    ms = np.zeros(2)
    sd.concordance_counts(ft, ct, lower, upper, kernel_ms=ms)
    assert np.all(ms > 0.0) and np.all(ms < 1e3)
    with pytest.raises(ValueError, match="out.pair"):
        sd.concordance_counts(f, c, lower, upper, out=sd.concordance_counts(f, c, lower[:1], upper[:1], device=True))


def _raw(hip, fine, coarse, M, n, ld, G, lower, upper, pair, all_, kept):
    return hip.lib().mlmc_concordance_counts(hip.ptr(fine), hip.ptr(coarse), M, n, ld, G, hip.ptr(lower), hip.ptr(upper), hip.ptr(pair),
                                             hip.ptr(all_), hip.ptr(kept), None)


def test_errors_and_no_ops(hip):
    import torch
    M, n, G = 3, 70, 2
    f = torch.zeros((M, n), dtype=torch.float64, device="cuda")
    lower, upper = np.full((G, M), -1.0), np.full((G, M), 1.0)
    pair = torch.zeros((G, 3, M, M), dtype=torch.int64, device="cuda")
    all_ = torch.zeros((G, 3), dtype=torch.int64, device="cuda")
    kept = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def fails(match, *args):
        assert _raw(hip, *args) != 0
        with pytest.raises(hip.MlmcHipError, match=match):
            hip.check(1)
    assert _raw(hip, f, None, M, n, n, G, lower, upper, pair, all_, kept) == 0
    assert kept.item() == n and torch.all(pair[:, 0] == n) and torch.all(pair[:, 1] == 0) and torch.all(all_[:, 2] == n)
    fails("above the cap", f, None, 1025, n, n, G, lower, upper, pair, all_, kept)
    fails("above the cap", f, None, M, n, n, 17, lower, upper, pair, all_, kept)
    fails("G >= 1", f, None, M, n, n, 0, lower, upper, pair, all_, kept)
    fails("G >= 1", f, None, -1, n, n, G, lower, upper, pair, all_, kept)
    fails("G >= 1", f, None, M, -1, n, G, lower, upper, pair, all_, kept)
    fails("row stride", f, None, M, n, n - 1, G, lower, upper, pair, all_, kept)
    fails("null fine", None, None, M, n, n, G, lower, upper, pair, all_, kept)
    fails("null limits", f, None, M, n, n, G, None, upper, pair, all_, kept)
    fails("null limits", f, None, M, n, n, G, lower, None, pair, all_, kept)
    fails("both counter arrays", f, None, M, n, n, G, lower, upper, None, None, kept)
    bad = lower.copy()
    bad[1, 2] = np.nan
    fails("event 1, component 2 is NaN", f, None, M, n, n, G, bad, upper, pair, all_, kept)
    fails("event 1, component 2 is NaN", f, None, M, n, n, G, lower, bad, pair, all_, kept)
    # nothing was added by a failed call; n = 0 and M = 0 are no-ops; either counter array and kept may be null
    assert _raw(hip, f, None, M, 0, 0, G, lower, upper, pair, all_, kept) == 0
    assert _raw(hip, None, None, 0, n, n, G, lower, upper, pair, all_, kept) == 0
    assert kept.item() == n and torch.all(pair[:, 0] == n) and torch.all(all_[:, 0] == n)
    assert _raw(hip, f, None, M, n, n, G, lower, upper, None, all_, None) == 0
    assert _raw(hip, f, None, M, n, n, G, lower, upper, pair, None, None) == 0
    assert kept.item() == n and torch.all(pair[:, 0] == 2 * n) and torch.all(all_[:, 0] == 2 * n)
