"""Covariance with variances of 49..64 Legendre moments: the pair levels' variance kernel (64 terms on the matrix cores) also sums
the differences of its 64 Legendre terms, the auxiliary Chebyshev pass of those levels walks the terms from 64 on only, and the first
64 Chebyshev sums follow from the row sums through the connection T_m = sum_k b_mk P_k (mlmc_chebyshev_connection_table).
Against the full auxiliary pass (MLMC_HIP_LINEARIZE_ROWSUMS=0) and against all three Gram matrices on the matrix cores
(MLMC_HIP_LINEARIZE=0): counts equal, second-moment sums bit-identical (the matrix accumulation and level 0 are the same code),
means within 1e-12 of sqrt(|sp| n), exact P_0 P_0 entries, bitwise reproducible, the same launch counts."""
import numpy as np
import pytest

from tests.util import level_arrays

pytestmark = pytest.mark.gpu
DOM = (-3.7190164854556804, 3.7190164854556804)
STEPS = [0.5, 0.07, 0.01, 0.03, 0.2]


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


def _levels(N, M, nan_every):
    """NaNs (level_arrays) and values outside the domain in both members of pairs, in every level"""
    lv = level_arrays(N, STEPS[:len(N)], M, nan_every)
    for f, c in lv:
        f[:, 7::53] = 5.0
        f[M - 1, 2::29] = -np.inf
        if c is not None:
            c[:, 11::61] = -4.5
            c[0, 5::23] = np.nan
    return lv


@pytest.fixture(scope="module")
def data():
    # 31 pairs: a single partial batch of the matrix kernel; 33: one full batch and one sample
    return {1: _levels([5301, 2500, 1777, 31, 33], 1, 19), 2: _levels([2800, 1100, 33], 2, 6)}


def _estimate(R, chunks, n_levels, n_comp=1, device=False):
    """chunks: [(level, fine[M, n], coarse[M, n] | None)] -> (n, n_rm, s, sp), (matrix-core launches, auxiliary launches)"""
    import torch
    from mlmc_amd import Legendre
    from mlmc_amd.engine import LevelAccumulator
    acc = LevelAccumulator(Legendre(R, DOM), n_levels, LevelAccumulator.COV, n_comp=n_comp)
    acc.kernel_time()
    acc.aux_kernel_time()
    keep = []
    for l, f, c in chunks:
        fa = np.ascontiguousarray(f if n_comp > 1 else f[0])
        ca = None if c is None else np.ascontiguousarray(c if n_comp > 1 else c[0])
        if device:
            fa = torch.from_numpy(fa).cuda()
            ca = None if ca is None else torch.from_numpy(ca).cuda()
            keep.append((fa, ca))
        acc.push(l, fa, ca)
    out = acc.finalize()
    launches = (acc.kernel_time()[1], acc.aux_kernel_time()[1])
    acc.close()
    return out, launches


def _check_against_the_other_routes(monkeypatch, R, chunks, n_levels, n_comp, device, pair):
    """pair[l]: level l holds pairs.  -> launches of the default route"""
    (n, n_rm, s, sp), launches = _estimate(R, chunks, n_levels, n_comp, device)
    again, _ = _estimate(R, chunks, n_levels, n_comp, device)
    for x, y in zip((n, n_rm, s, sp), again):
        assert np.array_equal(x, y)                              # bitwise reproducible
    for env in ("MLMC_HIP_LINEARIZE_ROWSUMS", "MLMC_HIP_LINEARIZE"):
        monkeypatch.setenv(env, "0")
        (n0, n_rm0, s0, sp0), launches0 = _estimate(R, chunks, n_levels, n_comp, device)
        monkeypatch.delenv(env)
        assert np.array_equal(n, n0) and np.array_equal(n_rm, n_rm0)
        if env == "MLMC_HIP_LINEARIZE_ROWSUMS":
            assert launches0 == launches                         # the switch changes no launch count
            assert np.array_equal(sp, sp0)
        else:
            assert launches0[1] == 0
            assert np.array_equal(sp[pair], sp0[pair])
        scale = np.sqrt(np.abs(sp0) * n[:, None]) + 1e-300
        err = np.max(np.abs(s - s0) / scale)
        print(R, n_comp, device, env, "s", err)
        assert err < 1e-12, err
    S = s.reshape(n_levels, n_comp, R, R)
    assert np.all(S[~pair][:, :, 0, 0] == n[~pair, None].astype(float)) and not S[pair][:, :, 0, 0].any()   # b_0k = delta_k0, d_0 = 0
    assert np.array_equal(S, S.transpose(0, 1, 3, 2))
    SP = sp.reshape(n_levels, n_comp, R, R)
    assert np.array_equal(SP, SP.transpose(0, 1, 3, 2))
    return launches


@pytest.mark.parametrize("R", [49, 64])
def test_row_sums_against_the_other_routes(hip, data, R, monkeypatch):
    """Every chunk on the linearised route (threshold 0); host and device chunks; one and two components (shared mask)."""
    monkeypatch.setenv("MLMC_HIP_LINEARIZE_MIN_N", "0")
    for n_comp in (1, 2):
        lv = data[n_comp]
        chunks = [(l, f, c) for l, (f, c) in enumerate(lv)]
        pair = np.array([c is not None for _, c in lv])
        for device in (False, True):
            launches = _check_against_the_other_routes(monkeypatch, R, chunks, len(lv), n_comp, device, pair)
            if device and n_comp == 1:       # one variance launch per pair level, three auxiliary launches: pair levels, level 0 twice
                assert launches == (len(lv) - 1, 3), launches


@pytest.mark.parametrize("R", [49, 64])
def test_row_sums_and_three_gram_chunks_in_one_level(hip, data, R, monkeypatch):
    """Threshold 2000: a pair level fed by a chunk of 2500 pairs (row sums) and one of 1777 (three Gram matrices) -- both add up."""
    monkeypatch.setenv("MLMC_HIP_LINEARIZE_MIN_N", "2000")
    lv = data[1]
    chunks = [(0, lv[0][0], None), (1, lv[1][0], lv[1][1]), (1, lv[2][0], lv[2][1]), (2, lv[3][0], lv[3][1])]
    pair = np.array([False, True, True])
    for device in (False, True):
        launches = _check_against_the_other_routes(monkeypatch, R, chunks, 3, 1, device, pair)
        assert launches[0] == 3                                  # the three pair chunks; level 0 without a matrix pass
