"""CPU tests of the joint sampling (Gaussian copula): the host side of tool.simple_distribution (correlation_factor, the argument
checks of joint_samples) and the NumPy restatement of the latent normals in tests/joint_sample_cases.py."""
import numpy as np
import pytest
from scipy import special

from tests import joint_sample_cases as jc
from tests import sample_cases as sc

SEED = 0x9E3779B97F4A7C15                            # of the sampling tests
FAR = 2 ** 33 + 1


def _sd():
    from mlmc_amd.tool import simple_distribution as sd
    return sd


def _random_corr(rng, M):
    A = rng.standard_normal((M, M + 3))
    c = A @ A.T
    d = 1.0 / np.sqrt(np.diag(c))
    c = c * d[:, None] * d[None, :]
    np.fill_diagonal(c, 1.0)
    return 0.5 * (c + c.T)


@pytest.mark.parametrize("M", [1, 2, 3, 12, 40])
def test_factor_of_a_positive_definite_matrix(M):
    """F F^T reproduces the matrix within M 2^-50, rows of unit norm, lower triangular, nothing repaired"""
    corr = _random_corr(np.random.default_rng(M), M)
    F, info = _sd().correlation_factor(corr)
    assert F.shape == (M, M) and F.dtype == np.float64 and F.flags.c_contiguous
    assert np.array_equal(F, np.tril(F))
    assert np.max(np.abs(F @ F.T - corr)) <= M * 2.0 ** -50
    assert np.max(np.abs(np.sum(F * F, axis=1) - 1.0)) <= 4 * 2.0 ** -52
    assert not info.repaired and info.max_change <= M * 2.0 ** -50
    assert abs(info.min_eig_in - np.linalg.eigvalsh(corr)[0]) <= 1e-12
    assert type(info).__name__ == "CorrelationFactorInfo" and info._fields == ("min_eig_in", "repaired", "max_change")


def test_factor_of_the_three_by_three_case():
    F, info = _sd().correlation_factor(jc.CORR3)
    assert np.max(np.abs(F @ F.T - jc.CORR3)) <= 3 * 2.0 ** -50 and not info.repaired
    assert np.allclose(np.linalg.eigvalsh(jc.CORR3), [0.137, 0.822, 2.04], atol=2e-3)


def test_indefinite_matrix_is_repaired():
    """off-diagonals 0.9, 0.9, -0.9: smallest eigenvalue -0.8; the result has a unit diagonal and eigenvalues >= min_eig"""
    corr = np.array([[1.0, 0.9, 0.9], [0.9, 1.0, -0.9], [0.9, -0.9, 1.0]])
    for min_eig in (1e-10, 1e-3):
        F, info = _sd().correlation_factor(corr, min_eig=min_eig)
        used = F @ F.T
        assert info.repaired and info.min_eig_in == pytest.approx(-0.8, abs=1e-12)
        assert np.max(np.abs(np.diag(used) - 1.0)) <= 4 * 2.0 ** -52
        # the rescaling to a unit diagonal divides by entries of at most 1 + |min_eig_in|: it can only shrink an eigenvalue by
        # that factor; rounding of the eigendecomposition and the factorisation is of the order 1e-15
        assert np.linalg.eigvalsh(used)[0] >= min_eig / 1.8 - 1e-14
        assert np.array_equal(F, np.tril(F)) and np.all(np.isfinite(F))
        assert info.max_change == pytest.approx(np.max(np.abs(used - corr)), abs=1e-15) and 0.1 < info.max_change < 1.0
    # a merely semi-definite matrix (rank 1) is repaired as well
    F, info = _sd().correlation_factor(np.ones((3, 3)))
    assert info.repaired and np.all(np.isfinite(F)) and info.max_change < 1e-8


def test_factor_symmetrises():
    corr = jc.CORR3.copy()
    corr[0, 1] += 1e-3
    corr[1, 0] -= 1e-3
    F, _ = _sd().correlation_factor(corr)
    assert np.max(np.abs(F @ F.T - jc.CORR3)) <= 3 * 2.0 ** -50


def test_factor_errors():
    sd = _sd()
    with pytest.raises(ValueError, match="square"):
        sd.correlation_factor(np.ones((2, 3)))
    with pytest.raises(ValueError, match="square"):
        sd.correlation_factor(np.ones(3))
    bad = jc.CORR3.copy()
    bad[0, 2] = np.nan
    with pytest.raises(ValueError, match="finite"):
        sd.correlation_factor(bad)
    bad = jc.CORR3.copy()
    bad[1, 1] = 1.0 + 1e-6
    with pytest.raises(ValueError, match="unit diagonal"):
        sd.correlation_factor(bad)


def test_joint_samples_argument_errors():
    """checked before anything touches the device"""
    sd = _sd()
    with pytest.raises(ValueError, match="exactly one of corr and factor"):
        sd.joint_samples([object()] * 3, 10, 1)
    with pytest.raises(ValueError, match="exactly one of corr and factor"):
        sd.joint_samples([object()] * 3, 10, 1, corr=jc.CORR3, factor=np.eye(3))
    for seed in (None, -1, 2 ** 64, 1.5, True):
        with pytest.raises(ValueError, match="seed"):
            sd.joint_samples([object()] * 3, 10, seed, corr=jc.CORR3)
    with pytest.raises(ValueError, match="n must be"):
        sd.joint_samples([object()] * 3, -1, 1, corr=jc.CORR3)
    with pytest.raises(ValueError, match=r"\[M, K\]"):
        sd.joint_samples([object()] * 2, 10, 1, corr=jc.CORR3)
    with pytest.raises(ValueError, match="streams"):
        sd.joint_samples([object()] * 3, 10, 1, corr=jc.CORR3, streams=[0, 1])


def test_entry_is_declared():
    import os
    from mlmc_amd import _lib
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "include", "mlmc_hip.h")).read()
    name = "mlmc_density_sample_joint_batch"
    assert name in text.split("#define MLMC_ABI_VERSION")[1].split("*/")[0]
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 21
    assert hasattr(_lib.load(), name)


def test_ndtri_route_agrees_with_mpmath():
    """200 uniforms of the sampling entry's form, the two extreme ones among them: scipy's ndtri against mpmath at 50 digits.
    Cephes documents a peak relative error of 7.2e-16 = 6.5 units of 2^-53 for ndtri; the bound is 16 units of
    2^-53 max(1, |z|)."""
    u = np.concatenate([[jc.U_LO, jc.U_HI, 0.5 - jc.U, 0.5 + jc.U], sc.uniforms(SEED, 3, FAR, 196)])
    assert np.all((u > 0) & (u < 1)) and u.size == 200
    z = special.ndtri(u)
    units = jc.z_units(z, jc.mp_ndtri(u))
    print(f"\nndtri against mpmath: worst {units.max():.3g} units at u = {u[int(np.argmax(units))]!r}")
    assert np.all(np.isfinite(z)) and units.max() <= 16
    assert abs(z[0] + z[1]) <= 16 * jc.U * abs(z[0]) and -8.3 < z[0] < -8.2
    # the antithetic normals are exact negations, and the even draws are the normals of index k
    both = jc.normals(SEED, [0, 7], 4, 10, antithetic=True)
    plain = jc.normals(SEED, [0, 7], 2, 5)
    assert np.array_equal(both[:, ::2], plain) and np.array_equal(both[:, 1::2], -plain)


@pytest.mark.parametrize("first", [0, FAR])
def test_restatement_statistics(first):
    """n = 16384 draws of the 3 x 3 case from the restated normals: the sample correlations of y = F z lie within 5 standard errors
    (1 - rho^2) / sqrt(n - 1) of rho, and every row of Phi(y) is within the DKW bound at confidence 1 - 1e-9 of uniform"""
    F, _ = _sd().correlation_factor(jc.CORR3)
    z = jc.normals(SEED, range(3), first, sc.DKW_N)
    y = F @ z
    errs = jc.correlation_errors(y, jc.CORR3)
    dist = [sc.kolmogorov_distance(special.ndtr(row)) for row in y]
    print(f"\nfirst = {first}: correlations {errs.max():.3g} standard errors, Kolmogorov distance {max(dist):.4f} (bound {sc.DKW_BOUND:.5f})")
    assert errs.max() <= 5.0
    assert max(dist) <= sc.DKW_BOUND
