"""GPU tests of the level diagnostics: mlmc_level_diagnostics against the long-double reference (tests/level_diag_ref.py),
determinism (run to run, a component alone and inside its vector, chunked and unchunked storages), Estimate
.estimate_level_diagnostics against the scalar estimates and the reference values of the six-component fixture, ABI errors.

Accuracy gate (tests/level_diag_ref.py): counts exact; means within 4 units of 2^-53 (|mean| + sd); every central sum within 32
units of 2^-53 sum |x - mean|^k (co-moment: sum |f - mean f| |c - mean c|).  The 32 is the worst value, 4.9 units, of an fp64 NumPy
twin of the two-pass form on such inputs (blocked in-order lane sums, a binary tree, the correction by S1 / n; the twin is not
part of the tree) with about 6 x for another summation order; it is 10^13 below what raw power sums show on the offset inputs.
Worst observed on an MI355X: 1.37 units in a mean, 4.74 in a central sum."""
import ctypes as C

import numpy as np
import pytest

from tests import level_diag_ref as ref
from tests.test_gpu_density_batch import _vector_levels, _vector_storage

pytestmark = pytest.mark.gpu

KINDS = ("normal", "offset", "sorted", "lognormal", "half_constant", "nan_fine", "nan_coarse", "nan_both", "all_nan", "one_kept")


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


def _rows(kind, n, rng):
    """fine [n], coarse [n] of one component"""
    z, w = rng.standard_normal(n), rng.standard_normal(n)
    f, c = z + 0.1 * w, z.copy()
    if kind == "offset":
        f, c = 1e6 + 1e-3 * z, 1e6 + 1e-3 * (z + 0.3 * w)
    elif kind == "sorted":
        f, c = np.sort(1e8 + z), np.sort(1e8 + w)
    elif kind == "lognormal":
        f, c = np.exp(2.0 * z), np.exp(2.0 * (z + 0.05 * w))
    elif kind == "half_constant":
        f[:n // 2] = 1.25
        c[:n // 2] = 0.75
    elif kind == "nan_fine":
        f[1::7] = np.nan
    elif kind == "nan_coarse":
        c[::5] = np.nan
    elif kind == "nan_both":
        f[2::11] = np.nan
        c[::3] = np.nan
    elif kind == "all_nan":
        f[:] = np.nan
    elif kind == "one_kept":
        f[:n - 1] = np.nan                               # the last sample alone survives (n = 1: the only one)
        c[:n // 2] = np.nan
    return f, c


def _levels(M, ns, seed):
    rng = np.random.default_rng(seed)
    levels = []
    for l, n in enumerate(ns):
        f, c = np.empty((M, n)), np.empty((M, n))
        for m in range(M):
            f[m], c[m] = _rows(KINDS[m % len(KINDS)], n, rng)
        levels.append((f, None if l == 0 else c))
    return levels


def _entry(hip, M, n_levels, chunks, outputs=True):
    """mlmc_level_diagnostics on chunks [(level, fine [M, n] | None, coarse [M, n] | None)] -> n, n_rm, stats"""
    import torch
    keep, fp, cp, lv, nn = [], [], [], [], []
    for level, f, c in chunks:
        tf = None if f is None else torch.from_numpy(np.ascontiguousarray(f)).cuda()
        tc = None if c is None else torch.from_numpy(np.ascontiguousarray(c)).cuda()
        keep.append((tf, tc))
        fp.append(None if tf is None else tf.data_ptr())
        cp.append(None if tc is None else tc.data_ptr())
        lv.append(level)
        nn.append(0 if f is None else f.shape[-1])
    torch.cuda.synchronize()
    nc = len(chunks)
    lv, nn = np.array(lv, dtype=np.int32), np.array(nn, dtype=np.int64)
    fa, ca = (C.c_void_p * max(nc, 1))(*fp), (C.c_void_p * max(nc, 1))(*cp)
    n = np.full((n_levels, max(M, 1)), -1, dtype=np.int64)
    n_rm = np.full((n_levels, max(M, 1)), -1, dtype=np.int64)
    stats = np.zeros((n_levels, max(M, 1), 9))
    hip.check(hip.lib().mlmc_level_diagnostics(M, n_levels, nc, hip.ptr(lv), C.cast(fa, C.c_void_p), C.cast(ca, C.c_void_p),
                                               hip.ptr(nn), hip.ptr(n) if outputs else None, hip.ptr(n_rm), hip.ptr(stats)))
    return n, n_rm, stats


N_TRIPLES = [(1, 2, 63), (64, 65, 255), (256, 257, 1023), (4097, 20011, 65)]


@pytest.mark.parametrize("M", [1, 3, 17])
@pytest.mark.parametrize("ns", N_TRIPLES)
def test_entry_against_the_long_double_reference(hip, M, ns):
    levels = _levels(M, ns, seed=1000 * M + ns[0])
    n, n_rm, stats = _entry(hip, M, 3, [(l, f, c) for l, (f, c) in enumerate(levels)])
    n0, n_rm0, want, scale = ref.levels_stats(levels)
    assert np.array_equal(n, n0) and np.array_equal(n_rm, n_rm0)
    um, us = ref.worst_units(stats, want, scale)
    print("M = %d, n = %s: worst mean %.2f units, worst central sum %.2f units" % (M, ns, um, us))
    assert um <= ref.GATE_MEAN and us <= ref.GATE_SUM
    assert np.all(np.isnan(stats[0, :, 6:]))                                   # level 0: no coarse statistics
    for l in range(3):
        for m in range(M):
            if n[l, m] == 0:
                assert np.all(np.isnan(stats[l, m]))
            if n[l, m] == 1:                                                   # the means are the values, every M is 0
                assert np.all(stats[l, m, [1, 2, 3, 5]] == 0.0) and stats[l, m, 0] == want[l, m, 0]
    if M == 17:
        assert n[1, 8] == 0 and n[1, 9] == 1 and n[0, 9] == 1


def test_infinite_values_are_values(hip):
    """a kept +-inf: counts as usual, the means it enters are +-inf as estimate_mean gives them (NaN where both signs meet), its
    central sums NaN; the other statistics and components are untouched -- in one chunk and merged from two"""
    rng = np.random.default_rng(9)
    n = 700
    f, c = rng.standard_normal((3, n)), rng.standard_normal((3, n))
    f0, c0 = f.copy(), c.copy()
    f[0, 5] = np.inf                                     # fine only
    f[1, 650], f[1, 3] = np.inf, -np.inf                 # both signs: no mean
    for chunks in ([(0, f, None), (1, f, c)], [(0, f[:, :300], None), (0, f[:, 300:], None), (1, f[:, :300], c[:, :300]),
                                              (1, f[:, 300:], c[:, 300:])]):
        n_k, n_rm, stats = _entry(hip, 3, 2, chunks)
        assert np.all(n_k == n) and np.all(n_rm == 0)
        for l in (0, 1):
            assert stats[l, 0, 0] == np.inf and stats[l, 0, 4] == np.inf and np.all(np.isnan(stats[l, 0, [1, 2, 3, 5]]))
            assert np.isnan(stats[l, 1, 0]) and np.isnan(stats[l, 1, 4])
        assert np.isnan(stats[1, 0, 8])
        _, _, want, scale = ref.levels_stats([(f0, None), (f0, c0)])
        u = ref.units(stats[:, 2], want[:, 2], scale[:, 2])                 # the finite component
        assert np.max(u[:, ref.MEAN_IDX]) <= ref.GATE_MEAN and np.max(u[:, ref.SUM_IDX]) <= ref.GATE_SUM
        uc = ref.units(stats[1, 0], want[1, 0], scale[1, 0])                # the coarse column of component 0 is finite
        assert uc[6] <= ref.GATE_MEAN and uc[7] <= ref.GATE_SUM


def test_more_samples_per_block_than_the_minimum(hip):
    """n > 1024 x 2048: the sample blocks grow beyond their least size (another block size, 1024 blocks per component)"""
    rng = np.random.default_rng(4)
    n = 1024 * 2048 + 4001
    z = rng.standard_normal((2, n))
    f = np.stack([1e6 + 1e-3 * z[0], np.exp(z[1])])
    c = np.stack([1e6 + 1e-3 * (z[0] + 0.3 * rng.standard_normal(n)), np.exp(0.9 * z[1])])
    f[1, 5::1001] = np.nan
    levels = [(f[:, :100], None), (f, c)]
    n_k, n_rm, stats = _entry(hip, 2, 2, [(0, f[:, :100], None), (1, f, c)])
    n0, n_rm0, want, scale = ref.levels_stats(levels)
    assert np.array_equal(n_k, n0) and np.array_equal(n_rm, n_rm0)
    um, us = ref.worst_units(stats, want, scale)
    print("n = %d: worst mean %.2f units, worst central sum %.2f units" % (n, um, us))
    assert um <= ref.GATE_MEAN and us <= ref.GATE_SUM


@pytest.fixture(scope="module")
def fixture_reference():
    levels, steps = _vector_levels()
    return ref.levels_stats(levels) + (steps,)


def _route(chunk_size):
    from mlmc_amd.quantity.quantity import make_root_quantity
    st, spec = _vector_storage(chunk_size)
    return st, make_root_quantity(st, spec)['q']


def test_determinism(hip, fixture_reference):
    from mlmc_amd.estimator import scalar_component
    from mlmc_amd.quantity import quantity_estimate as qe
    n0, n_rm0, want, scale, _ = fixture_reference
    results = {}
    for chunk_size in (None, 1500):
        st, root = _route(chunk_size)
        n, n_rm, stats = qe.level_diagnostics(root)
        n2, n_rm2, stats2 = qe.level_diagnostics(root)
        assert np.array_equal(n, n2) and np.array_equal(n_rm, n_rm2) and stats.tobytes() == stats2.tobytes()
        for m in range(6):                                # a component alone: the same bits as inside the vector
            n1, n_rm1, stats1 = qe.level_diagnostics(scalar_component(root, m))
            assert n1.shape == (3, 1) and stats1.shape == (3, 1, 9)
            assert np.array_equal(n1[:, 0], n[:, m]) and np.array_equal(n_rm1[:, 0], n_rm[:, m]), (chunk_size, m)
            assert stats1[:, 0].tobytes() == np.ascontiguousarray(stats[:, m]).tobytes(), (chunk_size, m)
        assert np.array_equal(n, n0) and np.array_equal(n_rm, n_rm0)
        um, us = ref.worst_units(stats, want, scale)
        print("fixture, chunk_size = %s: worst mean %.2f units, worst central sum %.2f units" % (chunk_size, um, us))
        assert um <= ref.GATE_MEAN and us <= ref.GATE_SUM
        results[chunk_size] = n
    assert np.array_equal(results[None], results[1500])


def test_api_on_the_vector_fixture(hip, fixture_reference):
    from mlmc_amd import diagnostics
    from mlmc_amd.estimator import Estimate, scalar_component
    from mlmc_amd.quantity import quantity_estimate as qe
    from tests.util import close
    n0, _, want, _, steps = fixture_reference
    st, root = _route(1500)
    d = Estimate(root, st).estimate_level_diagnostics()          # no moments function
    assert isinstance(d, diagnostics.LevelDiagnostics)
    assert d.n_samples.dtype == np.int64 and np.array_equal(d.n_samples, n0)
    for name in d.FIELDS[1:]:
        v = getattr(d, name)
        assert v.shape == (3, 6) and v.dtype == np.float64, name
    assert np.array_equal(d.level_steps, steps) and d.n_ops.shape == (3,)
    assert d.mlmc_mean.shape == d.mlmc_var.shape == (6,)
    for m in range(6):
        r = qe.estimate_mean(scalar_component(root, m))
        assert np.array_equal(d.n_samples[:, m], r.n_samples)
        assert close(d.mean_diff[:, m], r.l_means) and close(d.var_diff[:, m], r.l_vars), m
        assert close(d.mlmc_mean[m], r.mean) and close(d.mlmc_var[m], r.var), m
    # the long-double statistics of the fixture
    dref = diagnostics.from_central_sums(n0, want.astype(np.float64), level_steps=steps)
    for name in d.FIELDS[1:]:
        assert np.allclose(getattr(d, name), getattr(dref, name), rtol=1e-10, atol=1e-12, equal_nan=True), name
    flags = d.flags()
    assert flags.dtype == bool and flags.shape == (3, 6)
    assert not flags[:, :5].any() and flags[:, 5].all()
    assert np.all(np.abs(d.kurtosis_diff[:, 5] - [119.0, 146.0, 148.0]) < 0.5)       # the fine-only outliers of component 5
    assert np.all(np.abs(d.consistency[1:, 5] - [2.09, 1.15]) < 0.005)
    assert np.all(d.kurtosis_diff[:, :5] > 2.4) and np.all(d.kurtosis_diff[:, :5] < 8.2)
    assert np.all(d.consistency[1:, :5] <= 0.25) and np.all(np.isnan(d.consistency[0]))
    rates = d.rates()
    assert np.all(rates.beta[:4] >= 1.9) and np.all(rates.beta[:4] <= 2.1)
    assert rates.alpha.shape == rates.beta.shape == rates.bias.shape == (6,) and np.isfinite(rates.gamma)
    # a scalar quantity gives one column
    d1 = Estimate(scalar_component(root, 2), st).estimate_level_diagnostics()
    assert d1.kurtosis_diff.shape == (3, 1) and np.array_equal(d1.kurtosis_diff[:, 0], d.kurtosis_diff[:, 2])


def test_argument_errors_name_the_entry(hip):
    f = np.zeros((2, 100))
    n, n_rm, stats = _entry(hip, 2, 2, [(0, f, None), (1, f, f)])
    assert np.array_equal(n, np.full((2, 2), 100)) and np.array_equal(n_rm, np.zeros((2, 2)))
    assert np.all(stats[:, :, :4] == 0.0) and np.all(np.isnan(stats[0, :, 6:])) and np.all(stats[1, :, 6:] == 0.0)
    with pytest.raises(hip.MlmcHipError, match="mlmc_level_diagnostics: bad M"):
        _entry(hip, 0, 2, [(0, f, None)])
    with pytest.raises(hip.MlmcHipError, match="mlmc_level_diagnostics: null argument"):
        _entry(hip, 2, 2, [(0, f, None)], outputs=False)
    for level in (-1, 2):
        with pytest.raises(hip.MlmcHipError, match="mlmc_level_diagnostics: chunk level out of range"):
            _entry(hip, 2, 2, [(0, f, None), (level, f, f)])
    with pytest.raises(hip.MlmcHipError, match="mlmc_level_diagnostics: level 1 has chunks with and without coarse samples"):
        _entry(hip, 2, 2, [(0, f, None), (1, f, f), (1, f, None)])
    # a level without a chunk, a chunk without samples: counts 0, statistics NaN
    n, n_rm, stats = _entry(hip, 2, 3, [(0, f, None), (2, None, None)])
    assert np.array_equal(n[1:], np.zeros((2, 2))) and np.all(np.isnan(stats[1:]))
