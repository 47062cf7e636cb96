"""Covariance with variances of 17..128 Legendre moments: the inner accumulators of the linearised route sum Chebyshev
polynomials (one FMA per term; tables composed with the connection P_k = sum_m a_km T_m) wherever the mean-only term-split
kernel runs them.  The default route against all three Gram matrices on the matrix cores (MLMC_HIP_LINEARIZE=0) and against
Legendre sums (MLMC_HIP_LINEARIZE_CHEB=0) under the gates of test_covariance_mean_through_the_product_linearisation; the
benchmark's own route (default thresholds, chunks above them) against the C oracle."""
import numpy as np
import pytest

from oracle import oracle_c, oracle_np as onp
from tests.util import close, level_arrays

pytestmark = pytest.mark.gpu
DOM = (-3.7190164854556804, 3.7190164854556804)


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


def _estimate(fn, lv, n_comp=1, device=False):
    """-> (n, n_rm, s, sp), (matrix-core launches, auxiliary moments launches)"""
    import torch
    from mlmc_amd.engine import LevelAccumulator
    acc = LevelAccumulator(fn, len(lv), LevelAccumulator.COV, n_comp=n_comp)
    acc.kernel_time()
    acc.aux_kernel_time()
    keep = []
    for l, (f, c) in enumerate(lv):
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


@pytest.mark.parametrize("R", [17, 32, 33, 64, 100, 128])
def test_chebyshev_sums_against_the_other_routes(hip, R, monkeypatch):
    """Counts identical; pair-level second-moment sums bit-identical (the matrix kernels are the same); means within 1e-12 of
    sqrt(|sp| n); level-0 second moments (<= 64 moments: from 4 R - 3 level sums) within 1e-11.  Host and device chunks, and a
    two-component quantity (shared mask: the kernels with the run-time switches)."""
    from mlmc_amd import Legendre
    levels = level_arrays([5301, 2500, 1777] if R <= 64 else [901, 500, 377], [0.5, 0.07, 0.01], 1, 19)
    lv2 = level_arrays([2800, 1100] if R <= 64 else [700, 300], [0.3, 0.02], 2, 6)
    monkeypatch.setenv("MLMC_HIP_LINEARIZE_MIN_N", "0")
    for lv, n_comp, device in ((levels, 1, False), (levels, 1, True), (lv2, 2, False), (lv2, 2, True)):
        fn = Legendre(R, DOM)
        (n, n_rm, s, sp), launches = _estimate(fn, lv, n_comp, device)
        assert launches[1] > 0                                   # the linearised route was taken
        again, _ = _estimate(fn, lv, n_comp, device)
        for x, y in zip((n, n_rm, s, sp), again):
            assert np.array_equal(x, y)                          # bitwise reproducible
        pair = np.array([c is not None for _, c in lv])
        for env in ("MLMC_HIP_LINEARIZE", "MLMC_HIP_LINEARIZE_CHEB"):
            monkeypatch.setenv(env, "0")
            (n0, n_rm0, s0, sp0), launches0 = _estimate(Legendre(R, DOM), lv, n_comp, device)
            monkeypatch.delenv(env)
            assert (launches0[1] > 0) == (env == "MLMC_HIP_LINEARIZE_CHEB")
            assert np.array_equal(n, n0) and np.array_equal(n_rm, n_rm0)
            assert np.array_equal(sp[pair], sp0[pair])
            if R > 64:
                assert np.array_equal(sp, sp0)
            else:
                big = np.max(np.abs(sp0[~pair]), axis=1, keepdims=True)
                err = np.max(np.abs(sp[~pair] - sp0[~pair]) / np.maximum(np.abs(sp0[~pair]), 1e-3 * big))
                print(R, env, "level-0 sp", err)
                assert err < 1e-11, err
            scale = np.sqrt(np.abs(sp0) * n[:, None]) + 1e-300
            err = np.max(np.abs(s - s0) / scale)
            print(R, env, "s", err)
            assert err < 1e-12, err
        S = s.reshape(len(lv), n_comp, R, R)
        assert np.all(S[0, :, 0, 0] == float(n[0])) and not S[1:, :, 0, 0].any()     # exact counts: c'_00m = delta_m0


def test_headline_route_against_the_c_oracle(hip):
    """5 levels x 1.5e5 samples, 64 moments, default settings: every chunk is above the threshold of the linearised route (1e5
    samples at 33..64 moments) -- the benchmark's route: four variance-only matrix launches, one Chebyshev pass of 127 terms over
    the pair levels and two windows of 253 terms at level 0.  Against the C oracle under the project's 1e-10 gate, counts exact."""
    from mlmc_amd import Legendre
    L, N, R = 5, 150000, 64
    steps = [s[0] for s in onp.determine_level_parameters(L, [0.5, 0.01])]
    lv = []
    for l in range(L):
        f, c = onp.synth_level_samples(l, N, steps)
        f[5::97] = np.nan
        lv.append((f[None], None if c is None else c[None]))
    (n, n_rm, s, sp), launches = _estimate(Legendre(R, DOM), lv, device=True)
    assert launches == (L - 1, 3), launches
    again, _ = _estimate(Legendre(R, DOM), lv, device=True)
    for x, y in zip((n, n_rm, s, sp), again):
        assert np.array_equal(x, y)
    b = onp.Basis(onp.LEGENDRE, R, DOM)
    for l, (f, c) in enumerate(lv):
        nk, nr, so, spo = oracle_c.cov_level(b, f[0], None if c is None else c[0])
        assert nk == n[l] and nr == n_rm[l]
        rms = np.sqrt(spo / max(nk, 1)) * nk
        with np.errstate(invalid="ignore"):             # (0 / 0 at the P_0 P_0 entry of a pair level)
            print(l, "s", np.nanmax(np.abs(s[l] - so) / np.maximum(np.abs(so), rms)), "sp", np.nanmax(np.abs(sp[l] - spo) / np.abs(spo)))
        assert close(s[l], so, rms, 1e-10) and close(sp[l], spo, None, 1e-10)
    S = s.reshape(L, R, R)
    assert S[0, 0, 0] == float(n[0]) and not S[1:, 0, 0].any()
