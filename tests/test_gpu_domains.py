"""GPU tests of the per-component domains: engine.row_percentiles (mlmc_percentiles_rows) bit for bit against NumPy and the
scalar engine.percentiles over both device paths (LDS sort, segmented radix select with its tie fallback), host / CUDA /
strided inputs, NaN policies and errors; Estimate.estimate_domains and estimator.estimate_domains against the loop of the
scalar methods over the components, on Memory and DeviceMemory storages and at M = 1024."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QS = [0, 0.01, 1, 25, 50, 99, 99.999, 100]


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


def _row(kind, n, rng):
    x = rng.normal(size=n)
    if kind == 1:
        x *= 1e-300                                  # down into the subnormals
    elif kind == 2:
        x[rng.integers(0, n, size=max(1, n // 9))] = np.nan
        x[0] = 0.5                                   # at least one valid value
    elif kind == 3:
        x[::11] = np.inf
        x[1::13] = -np.inf
        x[2::5] = 0.0
        x[3::7] = -0.0
    elif kind == 4:
        x = np.round(x, 1)                           # ties
    elif kind == 5:
        x[:] = 3.25                                  # constant
    elif kind == 6:
        x = -np.exp(x)                               # negative lognormal
    elif kind == 7:
        x = rng.choice([-1.0, 0.5, 2.0], size=n)     # three distinct values
    elif kind == 8 and n >= 2:                       # two clusters far apart: each rank pair straddles two key prefixes
        x[: n // 2] = rng.uniform(-2.0, -1.0, size=n // 2)
        x[n // 2:] = rng.uniform(1e6, 2e6, size=n - n // 2)
    return x


def _rows(M, n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([_row(m % 9, n, rng) for m in range(M)])


def _numpy_rows(x, qs=QS):
    with np.errstate(invalid="ignore"):
        return np.stack([np.percentile(r[~np.isnan(r)], qs) for r in x])


def _check(got, x):
    want = _numpy_rows(x)
    assert got.shape == want.shape
    bad = [m for m in range(x.shape[0]) if not np.array_equal(got[m], want[m], equal_nan=True)]
    assert not bad, (x.shape, bad[:5], got[bad[0]], want[bad[0]])


SHAPES = [(1, 1), (1, 3_000_001), (3, 2), (64, 4097), (1000, 255), (10_000, 100), (9, 40_000)]


@pytest.mark.parametrize("M,n", SHAPES)
def test_row_percentiles_bit_identical_to_numpy(hip, M, n):
    """Host array, CUDA tensor and a strided view (ld > n) of the same rows: every row bit for bit np.percentile of its
    non-NaN values; the rows also equal the scalar engine.percentiles."""
    import torch
    from mlmc_amd import engine
    x = _rows(M, n, seed=M * 7 + n)
    got = engine.row_percentiles(x, QS)
    _check(got, x)
    xd = torch.from_numpy(x).cuda()
    assert np.array_equal(engine.row_percentiles(xd, QS), got, equal_nan=True)
    wide = np.full((M, n + 5), 7.0e300)
    wide[:, :n] = x
    assert np.array_equal(engine.row_percentiles(wide[:, :n], QS), got, equal_nan=True)
    wd = torch.from_numpy(wide).cuda()[:, :n]
    assert wd.stride(0) == n + 5
    assert np.array_equal(engine.row_percentiles(wd, QS), got, equal_nan=True)
    step = 1 if M <= 1000 else 7
    for m in range(0, M, step):
        assert np.array_equal(engine.percentiles(x[m], QS), got[m], equal_nan=True), m


def test_row_percentiles_heavy_ties_take_all_digit_passes(hip):
    """Rows of 400 000 values rounded to integers (a 22-bit prefix holds far more values than the LDS finish takes), a constant
    long row, a long row of three values, beside ordinary long rows."""
    import torch
    from mlmc_amd import engine
    rng = np.random.default_rng(5)
    n = 400_000
    x = np.stack([np.round(rng.normal(size=n)), np.full(n, -2.5), rng.choice([-1.0, 0.5, 2.0], size=n),
                  rng.normal(size=n), np.round(rng.normal(size=n) * 3.0) * 1e-3])
    got = engine.row_percentiles(torch.from_numpy(x).cuda(), QS)
    _check(got, x)
    got1 = engine.row_percentiles(x[:1], QS)
    _check(got1, x[:1])
    assert np.array_equal(engine.percentiles(x[0], QS), got1[0])


def test_row_percentiles_many_percentiles(hip):
    """More percentiles than one radix round takes (long rows) and than the LDS path has threads to spare (short rows)."""
    from mlmc_amd import engine
    qs = np.linspace(0.0, 100.0, 77)
    for M, n in ((3, 20_000), (5, 300)):
        x = _rows(M, n, seed=n)
        got = engine.row_percentiles(x, qs)
        assert np.array_equal(got, _numpy_rows(x, qs), equal_nan=True), (M, n)


def test_row_percentiles_propagate(hip):
    from mlmc_amd import engine
    for M, n in ((50, 300), (4, 30_000)):
        x = _rows(M, n, seed=11)
        x[3, 7] = np.nan
        has_nan = np.isnan(x).any(axis=1)
        assert has_nan.any() and not has_nan.all()
        got = engine.row_percentiles(x, QS, nan_policy="propagate")
        assert np.all(np.isnan(got[has_nan]))
        assert np.array_equal(got[~has_nan], _numpy_rows(x[~has_nan]), equal_nan=True)   # (inf rows: NaN)
        for m in range(M):
            assert np.array_equal(got[m], engine.percentiles(x[m], QS, nan_policy="propagate"), equal_nan=True)


def test_row_percentiles_errors_then_recovery(hip):
    import ctypes as C
    from mlmc_amd import _lib, engine
    for M, n in ((20, 100), (3, 20_000)):
        x = _rows(M, n, seed=3)
        x[17 % M] = np.nan
        with pytest.raises(_lib.MlmcHipError, match="row {} has no non-NaN value".format(17 % M)):
            engine.row_percentiles(x, [1.0, 99.0])
        x[17 % M] = 1.0
        _check(engine.row_percentiles(x, QS), x)
    with pytest.raises(_lib.MlmcHipError, match="percentiles"):
        engine.row_percentiles(np.ones((2, 5)), [1.0, 101.0])
    x = np.ones((2, 5))
    out = np.empty((2, 2))
    q = np.array([1.0, 99.0])
    L = _lib.lib()
    for args in ((x, 2, 5, 4, q, 2), (x, 2, 5, 5, q, 0), (x, 0, 5, 5, q, 2), (x, 2, 0, 5, q, 2), (None, 2, 5, 5, q, 2)):
        xx, M, n, ld, qq, nq = args
        assert L.mlmc_percentiles_rows(_lib.ptr(xx), M, n, ld, _lib.ptr(qq), nq, _lib.ptr(out), None, _lib.HOST) != 0, args
        assert L.mlmc_last_error()
    nv = np.empty(2, dtype=np.int64)
    x[1, 2] = np.nan
    _lib.check(L.mlmc_percentiles_rows(_lib.ptr(x), 2, 5, 5, _lib.ptr(q), 2, _lib.ptr(out), _lib.ptr(nv), _lib.HOST))
    assert list(nv) == [5, 4] and np.array_equal(out, np.ones((2, 2)))
    assert C.sizeof(C.c_int64) == 8


# ---- domains of a vector quantity ----------------------------------------------------------------------------------------
def _levels(M, N, seed, off_comp=None):
    rng = np.random.default_rng(seed)
    out = []
    for l, n in enumerate(N):
        f = rng.normal(size=(M, n)) * (1.0 + 0.1 * np.arange(M))[:, None] + 0.2 * np.arange(M)[:, None]
        c = None if l == 0 else f + 0.05 * rng.normal(size=(M, n))
        if off_comp is not None:                              # far off the other components' range
            f[off_comp] = f[off_comp] * 1e3 + 5e4
            if c is not None:
                c[off_comp] = c[off_comp] * 1e3 + 5e4
        f[1 % M, 3::17] = np.nan
        out.append((f, c))
    return out


def _memory_storage(levels, spec, chunk_size=None):
    from mlmc_amd.sample_storage import Memory
    st = Memory(chunk_size=chunk_size)
    st.save_global_data(result_format=spec, level_parameters=[[0.1 ** (l + 1)] for l in range(len(levels))])
    for l, (f, c) in enumerate(levels):
        st.set_level_samples(l, f.T, None if c is None else c.T)
    return st


def _vector_spec():
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    return [QuantitySpec(name="a", unit="m", shape=(3, 1), times=[1, 2], locations=['0', '1']),
            QuantitySpec(name="b", unit="m", shape=(2, 1), times=[1, 2], locations=['0', '1'])]   # M = 12 + 8


def _loop(q, st, quantile=None, module=False):
    from mlmc_amd import estimator
    from mlmc_amd.estimator import Estimate, scalar_component
    fn = estimator.estimate_domain if module else Estimate.estimate_domain
    return np.array([fn(scalar_component(q, m), st, quantile) for m in range(int(q.size()))], dtype=float).reshape(-1, 2)


@pytest.mark.parametrize("chunk_size", [None, 700])
def test_estimate_domains_matches_the_loop_on_memory(hip, chunk_size):
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.quantity.quantity import make_root_quantity
    spec = _vector_spec()
    st = _memory_storage(_levels(20, [3000, 1100, 400], seed=1, off_comp=6), spec, chunk_size)
    qe.device_cache_clear()
    root = make_root_quantity(st, spec)
    for q in (root, root['a'], root['a'] * 2.0 + 1.0, root['b'][2]):
        for quantile in (None, 0.05):
            got = Estimate.estimate_domains(q, st, quantile)
            want = _loop(q, st, quantile)
            assert got.shape == (int(q.size()), 2)
            assert np.array_equal(got, want), (np.argwhere(got != want)[:4])
    doms = Estimate.estimate_domains(root, st)
    assert doms[6, 0] > 1e4                      # component 6 is far off: its own domain, not the pooled one
    # a scalar quantity gives [[lo, hi]]
    q0 = root['a'][1]['0'][1, 0]
    assert np.array_equal(Estimate.estimate_domains(q0, st), np.array([Estimate.estimate_domain(q0, st)]))


def test_estimate_domains_matches_the_loop_on_device_memory(hip):
    import torch
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    from mlmc_amd.sample_storage import DeviceMemory
    spec = [QuantitySpec(name="length", unit="m", shape=(4, 1), times=[1, 2, 3], locations=['0'])]
    levels = _levels(12, [5000, 2000, 900], seed=2, off_comp=3)
    dev = DeviceMemory()
    dev.save_global_data(result_format=spec, level_parameters=[[0.1], [0.01], [0.001]])
    for l, (f, c) in enumerate(levels):
        pairs = np.stack([f, np.zeros_like(f) if c is None else c], axis=-1)
        dev.set_level_samples(l, torch.from_numpy(pairs).cuda())
    qe.device_cache_clear()
    q = make_root_quantity(dev, spec)['length']
    got = Estimate.estimate_domains(q, dev)
    assert np.array_equal(got, _loop(q, dev))
    # the same samples in a host storage give the same domains
    st = _memory_storage(levels, spec)
    assert np.array_equal(Estimate.estimate_domains(make_root_quantity(st, spec)['length'], st), got)


def test_module_estimate_domains_matches_the_loop(hip):
    """NaN propagates per component: a component with a NaN in some level gets [nan, nan], the others their own range."""
    from mlmc_amd import estimator
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.quantity.quantity import make_root_quantity
    spec = _vector_spec()
    levels = _levels(20, [3000, 1100, 400], seed=4, off_comp=9)
    st = _memory_storage(levels, spec, 500)
    qe.device_cache_clear()
    root = make_root_quantity(st, spec)
    got = estimator.estimate_domains(root, st)
    want = _loop(root, st, module=True)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.all(np.isnan(got[1])) and not np.isnan(got[np.arange(20) != 1]).any()
    got = estimator.estimate_domains(root['a'] * 2.0 + 1.0, st, 0.1)
    assert np.array_equal(got, _loop(root['a'] * 2.0 + 1.0, st, 0.1, module=True), equal_nan=True)


def test_estimate_domains_raises_where_the_loop_raises(hip):
    from mlmc_amd import _lib
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.quantity.quantity import make_root_quantity
    spec = _vector_spec()
    levels = _levels(20, [300, 110], seed=6)
    levels[0][0][5] = np.nan                            # component 5 has no valid sample in level 0 (the chunk of every level)
    st = _memory_storage(levels, spec)
    qe.device_cache_clear()
    root = make_root_quantity(st, spec)
    with pytest.raises(_lib.MlmcHipError):
        _loop(root, st)
    with pytest.raises(_lib.MlmcHipError, match="row 5"):
        Estimate.estimate_domains(root, st)


def test_estimate_domains_at_size(hip):
    """M = 1024 components, 3 levels of 2 x 10^4 samples: the batched domains against NumPy on host copies."""
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    M, n = 1024, 20_000
    spec = [QuantitySpec(name="f", unit="m", shape=(512, 1), times=[1, 2], locations=['0'])]
    rng = np.random.default_rng(8)
    levels = []
    for l in range(3):
        f = rng.standard_normal((M, n)) * 0.5 + np.linspace(-3.0, 3.0, M)[:, None]
        f[::97, 11::113] = np.nan
        levels.append((f, None if l == 0 else f * 0.99))
    st = _memory_storage(levels, spec)
    qe.device_cache_clear()
    root = make_root_quantity(st, spec)['f']
    got = Estimate.estimate_domains(root, st)
    # the level-0 chunk for every level (the scalar method's chunks): per component, NumPy on the host copy
    f0 = levels[0][0]
    want = _numpy_rows(f0, [1.0, 99.0])
    assert np.array_equal(got, want)


def test_construct_densities_on_batched_domains(hip):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.quantity.quantity import make_root_quantity
    spec = _vector_spec()
    st = _memory_storage(_levels(20, [3000, 1100, 400], seed=9, off_comp=2), spec)
    qe.device_cache_clear()
    root = make_root_quantity(st, spec)['a']
    doms = Estimate.estimate_domains(root, st)
    doms_loop = _loop(root, st)
    assert np.array_equal(doms, doms_loop)
    est = Estimate(root, st, None)
    got = est.construct_densities(moments_fns=[Legendre(7, tuple(d)) for d in doms])
    want = est.construct_densities(moments_fns=[Legendre(7, tuple(d)) for d in doms_loop])
    for (d, info, res, m), (d0, info0, res0, m0) in zip(got, want):
        assert np.array_equal(d.multipliers, d0.multipliers) and info[1] == info0[1]
        assert np.array_equal(m.domain, m0.domain) and res.nit == res0.nit
