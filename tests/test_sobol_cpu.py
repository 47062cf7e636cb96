"""CPU tests of the scrambled Sobol' points behind MLMC_SAMPLE_SOBOL (include/mlmc_hip.h): the host entry mlmc_sobol_table against
SciPy's unscrambled sequence and against the NumPy restatement (tests/sobol_cases.py), the structure of the restatement's points,
the errors of the entry and of the Python layer.  No device is needed."""
import ctypes as C

import numpy as np
import pytest

from tests import sobol_cases as sb

SEEDS = (0, 1, 2 ** 63 + 5)
DIMS = (0, 1, 7, 1023)


@pytest.fixture(scope="module")
def lib():
    from mlmc_amd import _lib
    return _lib


def _table(lib, seed, scramble, dims):
    dims = np.ascontiguousarray(dims, dtype=np.uint32)
    dirs = np.full((dims.size, sb.BITS), 7, dtype=np.uint64)
    shift = np.full(dims.size, 7, dtype=np.uint64)
    rc = lib.load().mlmc_sobol_table(seed, scramble, lib.ptr(dims), dims.size, lib.ptr(dirs), lib.ptr(shift))
    return rc, dirs, shift


def test_raw_table_reproduces_scipy(lib):
    """the raw direction numbers of all 1024 dimensions, through the Gray-code formula, give the first 1024 points of
    scipy.stats.qmc.Sobol(1024, scramble=False, bits=52) bit for bit; the restatement's recurrence gives the same table"""
    from scipy.stats import qmc
    rc, dirs, shift = _table(lib, 3, 0, np.arange(sb.DIMS))
    lib.check(rc)
    assert not shift.any()
    got = sb.raw_points(dirs, np.arange(1024))                                         # [1024 dims, 1024 points]
    want = np.round(qmc.Sobol(sb.DIMS, scramble=False, bits=sb.BITS).random(1024) * 2.0 ** sb.BITS).astype(np.uint64)
    assert np.array_equal(got.T, want)
    assert np.array_equal(dirs, sb.raw_directions(np.arange(sb.DIMS)))
    # V[t] = m << (51 - t) with m odd and below 2^(t + 1)
    t = np.arange(sb.BITS, dtype=np.uint64)
    m = dirs >> (np.uint64(sb.BITS - 1) - t)
    assert np.array_equal(m << (np.uint64(sb.BITS - 1) - t), dirs) and np.all(m & np.uint64(1)) and np.all(m < (np.uint64(2) << t))


@pytest.mark.parametrize("seed", SEEDS)
def test_scrambled_table_is_the_restatement(lib, seed):
    rc, dirs, shift = _table(lib, seed, 1, DIMS)
    lib.check(rc)
    want_dirs, want_shift = sb.scrambled_table(seed, DIMS, sb.raw_directions(DIMS))
    assert np.array_equal(dirs, want_dirs) and np.array_equal(shift, want_shift)
    assert np.all(dirs < 2 ** sb.BITS) and np.all(shift < 2 ** sb.BITS)
    # the scramble is lower triangular with a unit diagonal: the leading digit of a value passes unchanged
    raw = sb.raw_directions(DIMS)
    assert np.array_equal(dirs >> np.uint64(sb.BITS - 1), raw >> np.uint64(sb.BITS - 1))
    from mlmc_amd.tool import simple_distribution as sd
    py_dirs, py_shift = sd.sobol_table(seed, DIMS)
    assert np.array_equal(py_dirs, dirs) and np.array_equal(py_shift, shift)
    raw_dirs, zero = sd.sobol_table(seed, DIMS, scramble=False)
    assert np.array_equal(raw_dirs, raw) and not zero.any()


@pytest.mark.parametrize("seed", SEEDS)
def test_structure_of_the_points(seed):
    """blocks of 4096 points aligned to 4096 hit each of the 4096 strata of every dimension once, dimensions (0, 1) each 64 x 64
    cell once; the direct formula agrees with Gray steps from 2^40"""
    for first in (0, 3 * 4096):
        m = sb.points(seed, DIMS, first, 4096)
        strata = (m >> np.uint64(sb.BITS - 12)).astype(np.int64)
        for row in strata:
            assert np.array_equal(np.sort(row), np.arange(4096))
        cells = (m[0] >> np.uint64(sb.BITS - 6)).astype(np.int64) * 64 + (m[1] >> np.uint64(sb.BITS - 6)).astype(np.int64)
        assert np.array_equal(np.sort(cells), np.arange(4096))
        u = sb.to_unit(m)
        assert np.all((u > 0) & (u < 1)) and np.array_equal(u * 2.0 ** 53 % 2, np.ones_like(u))
    dirs, shift = sb.scrambled_table(seed, DIMS, sb.raw_directions(DIMS))
    start = 2 ** 40
    direct = sb.points(seed, DIMS, start, 64)
    m = direct[:, 0].copy()
    for j in range(1, 64):
        i = start + j - 1                                   # the step from point i to i + 1 flips the bit ctz(i + 1) of the Gray code
        c = ((i + 1) & -(i + 1)).bit_length() - 1
        m = m ^ dirs[:, c]
        assert np.array_equal(m, direct[:, j]), j
    assert np.array_equal(sb.uniforms(seed, 7, 50, 100), sb.uniforms(seed, 7, 0, 150)[50:])
    assert not np.array_equal(sb.uniforms(seed, 7, 0, 64), sb.uniforms(seed + 1, 7, 0, 64))


def test_errors_of_the_host_entry(lib):
    def expect(rc, pattern):
        with pytest.raises(lib.MlmcHipError, match=pattern):
            lib.check(rc)
    L = lib.load()
    dims = np.array([0, 5], dtype=np.uint32)
    dirs, shift = np.zeros((2, sb.BITS), dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    P = lib.ptr
    assert L.mlmc_sobol_table(1, 1, P(dims), 2, P(dirs), P(shift)) == 0
    expect(L.mlmc_sobol_table(1, 1, None, 2, P(dirs), P(shift)), "mlmc_sobol_table: null")
    expect(L.mlmc_sobol_table(1, 1, P(dims), 2, None, P(shift)), "mlmc_sobol_table: null")
    expect(L.mlmc_sobol_table(1, 1, P(dims), 2, P(dirs), None), "mlmc_sobol_table: null")
    expect(L.mlmc_sobol_table(1, 1, P(dims), -1, P(dirs), P(shift)), "mlmc_sobol_table: nd < 0")
    expect(L.mlmc_sobol_table(1, 2, P(dims), 2, P(dirs), P(shift)), "mlmc_sobol_table: scramble")
    bad = np.array([0, 1024], dtype=np.uint32)
    expect(L.mlmc_sobol_table(1, 1, P(bad), 2, P(dirs), P(shift)), r"mlmc_sobol_table: dims\[1\] = 1024")
    dirs[:] = 7
    assert L.mlmc_sobol_table(1, 1, None, 0, None, None) == 0
    assert L.mlmc_sobol_table(1, 1, P(bad), 0, P(dirs), P(shift)) == 0 and np.all(dirs == 7)
    assert lib.SAMPLE_SOBOL == 8


def test_python_layer_refuses_qmc_with_antithetic():
    """every sampling entry raises before anything touches a device: the distributions are never looked at"""
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.tool import simple_distribution as sd
    from mlmc_amd.tool.distribution import Distribution
    kw = dict(antithetic=True, qmc=True)
    nothing = object()
    calls = [lambda: sd.samples([nothing], 4, 1, **kw),
             lambda: sd.joint_samples([nothing], 4, 1, factor=np.eye(1), **kw),
             lambda: sd.conditional_samples([nothing, nothing], 4, 1, {0: 0.0}, corr=np.eye(2), **kw),
             lambda: sd.SimpleDistribution.rvs(nothing, 4, 1, **kw),
             lambda: Distribution.rvs(nothing, 4, 1, **kw),
             lambda: Estimate.sample_components(nothing, 4, 1, **kw),
             lambda: Estimate.sample_joint(nothing, 4, 1, **kw),
             lambda: Estimate.sample_conditional(nothing, 4, 1, {0: 0.0}, **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="qmc and antithetic"):
            call()
