"""GPU tests of the multilevel walk and the public interface of the concordance counts: quantity_estimate.component_concordance
against the NumPy twin of tests/concordance_cases.py (integer for integer), Estimate.estimate_tail_dependence on the two copula
cases of that file and Estimate.estimate_joint_frequency."""
import numpy as np
import pytest
from scipy import special

from tests import concordance_cases as cc
from tests import score_cases as sk
from tests.test_gpu_normal_scores import _accumulation_levels, _closed_three, _densities, _estimate

pytestmark = pytest.mark.gpu
INF = np.inf
U_LOWER = np.array([[0.7, 0.7, 0.7], [-INF, -INF, -INF], [0.2, 0.1, 0.3]])
U_UPPER = np.array([[INF, INF, INF], [0.4, 0.4, 0.4], [0.9, 0.8, INF]])


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


def _uniform_three():
    """three uniform marginals on (0, 1): Fhat(x) = x up to the rounding of the quadrature"""
    return [sk.closed_distribution(0.0, (0.0, 1.0)) for _ in range(3)]


def _twin_levels(levels, lower, upper):
    counts = [cc.twin_counts(f, c, lower, upper) for f, c in levels]
    return (np.array([c[2] for c in counts]), np.array([c[0] for c in counts]), np.array([c[1] for c in counts]))


def test_walk_with_scores_equals_the_twin_on_the_uniforms(hip, monkeypatch):
    """component_concordance(scores=...) == the twin applied to the uniforms of normal_scores(return_uniforms=True), level by
    level; its n is the n_samples of estimate_score_correlation; the block width of the score route changes no bit"""
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.tool import simple_distribution as sd
    levels = _accumulation_levels()
    distrs = _closed_three()
    est = _estimate(levels)
    got = qe.component_concordance(est.quantity, U_LOWER, U_UPPER, scores=distrs)
    uniforms = []
    for f, c in levels:
        out = sd.normal_scores(distrs, f, c, return_uniforms=True)
        uniforms.append((out[1], None) if c is None else (out[2], out[3]))
    n, pair, all_ = _twin_levels(uniforms, U_LOWER, U_UPPER)
    assert np.array_equal(got.n, n) and np.array_equal(got.pair, pair) and np.array_equal(got.all, all_)
    assert np.array_equal(got.n_rm, np.array([f.shape[1] for f, _ in levels]) - n) and np.all(got.n_rm > 0)
    assert got.pair.shape == (3, 3, 3, 3, 3) and got.pair.dtype == np.int64 and got.pair[0, 0, 0].max() > 50
    res = est.estimate_score_correlation(densities=_densities(distrs))
    assert np.array_equal(got.n, res.n_samples) and np.array_equal(got.n_rm, res.n_rm_samples)
    monkeypatch.setenv("MLMC_SCORE_BLOCK_COLUMNS", "96")
    assert qe.score_block_columns(3) == 96
    blocks = qe.component_concordance(est.quantity, U_LOWER, U_UPPER, scores=distrs)
    assert all(np.array_equal(a, b) for a, b in zip(got, blocks))
    few = qe.component_concordance(est.quantity, U_LOWER, U_UPPER, scores=distrs, pairs=False)
    assert few.pair is None and np.array_equal(few.all, all_) and np.array_equal(few.n, n)
    with pytest.raises(ValueError, match="2 score distributions for 3 components"):
        qe.component_concordance(est.quantity, U_LOWER, U_UPPER, scores=distrs[:2])
    with pytest.raises(ValueError, match="NaN"):
        qe.component_concordance(est.quantity, np.nan, U_UPPER)


def test_host_chunks_equal_one_resident_tensor(hip, monkeypatch):
    """a store that hands a level out in host chunks of 32 samples gives the counts of the level as one resident tensor: the raw
    route, limits in the units of the components"""
    from mlmc_amd.quantity import quantity_estimate as qe
    from tests.test_gpu_estimate_walk import _quantity
    rng = np.random.default_rng(11)
    levels = []
    for l, n in enumerate((96, 48, 24)):
        f = rng.uniform(-0.9, 0.9, size=(2, n))
        c = None if l == 0 else np.clip(f + 0.2 * rng.standard_normal((2, n)), -0.95, 0.95)
        f[l % 2, 3::9] = np.nan
        levels.append((f, c))
    lower, upper = np.array([[0.0, -0.5], [-INF, 0.2]]), np.array([[INF, 0.5], [0.1, INF]])
    n, pair, all_ = _twin_levels(levels, lower, upper)
    qe.device_cache_clear()
    _, q = _quantity(levels)
    resident = qe.component_concordance(q, lower, upper)
    assert np.array_equal(resident.n, n) and np.array_equal(resident.pair, pair) and np.array_equal(resident.all, all_)
    monkeypatch.setenv("MLMC_HIP_DEVICE_CACHE_GB", "0")
    monkeypatch.setenv("MLMC_HIP_DEVICE_TREE", "0")
    qe.device_cache_clear()
    _, q = _quantity(levels, chunk_size=32)
    chunked = qe.component_concordance(q, lower, upper)
    assert all(np.array_equal(a, b) for a, b in zip(resident, chunked))
    qe.device_cache_clear()


@pytest.fixture(scope="module")
def gauss_estimate(hip):
    return _estimate(cc.copula_levels("gauss"))


def _diagonal_z(res, probs):
    M = res.prob.shape[-1]
    i = np.arange(M)
    return (res.prob[:, i, i] - (1.0 - np.asarray(probs))[:, None]) / np.sqrt(res.var[:, i, i])


def test_gaussian_copula_passes(gauss_estimate):
    res = gauss_estimate.estimate_tail_dependence(probs=cc.PROBS, corr=cc.CORR, densities=_densities(_uniform_three()))
    z, dz = cc.off_diagonal(res.z), _diagonal_z(res, cc.PROBS)
    print(f"\nGaussian copula end to end: z = {np.array2string(z, precision=4)}, diagonal {np.array2string(dz, precision=3)}")
    assert np.all(np.abs(z) < cc.Z_BOUND) and np.all(np.abs(dz) < cc.Z_BOUND)
    assert res.prob.shape == res.var.shape == res.chi.shape == res.model.shape == res.chi_model.shape == res.z.shape == (2, 3, 3)
    assert np.all(np.isnan(res.z[:, np.arange(3), np.arange(3)])) and np.array_equal(res.z, res.z.transpose(0, 2, 1), equal_nan=True)
    assert np.array_equal(res.marginal, res.prob[:, np.arange(3), np.arange(3)])
    assert np.array_equal(res.model, cc.model_orthant(cc.PROBS, cc.CORR))
    assert np.array_equal(res.chi, res.prob / (1.0 - np.array(cc.PROBS))[:, None, None])
    assert np.array_equal(res.n_samples, [cc.N_LEVEL, cc.N_LEVEL]) and np.array_equal(res.n_rm_samples, [0, 0])
    assert np.array_equal(res.corr, cc.CORR) and res.counts.pair.shape == (2, 2, 3, 3, 3)
    # the statistics are those of the twin from the counts; the frequencies are the twin's on the same uniforms up to the samples
    # within a rounding of Fhat(x) = x of a level
    _, _, prob, var = cc.twin_level_statistics(res.n_samples, res.counts.pair)
    assert np.array_equal(res.prob, prob) and np.allclose(res.var, var, rtol=1e-13, atol=0)
    assert np.allclose(z, cc.Z_GAUSS, rtol=0, atol=0.05)
    # corr="scores" resolves like sample_joint: the verdict stays
    scored = gauss_estimate.estimate_tail_dependence(probs=cc.PROBS, corr="scores", densities=_densities(_uniform_three()))
    assert np.array_equal(scored.prob, res.prob) and np.max(np.abs(scored.corr - cc.CORR)) < 0.01
    assert np.all(np.abs(cc.off_diagonal(scored.z)) < cc.Z_BOUND)
    with pytest.raises(ValueError, match="tail must be"):
        gauss_estimate.estimate_tail_dependence(tail="left", corr=cc.CORR, densities=_densities(_uniform_three()))
    with pytest.raises(ValueError, match="probability levels"):
        gauss_estimate.estimate_tail_dependence(probs=(0.9, 1.0), corr=cc.CORR, densities=_densities(_uniform_three()))


def test_student_t_copula_is_found(hip):
    est = _estimate(cc.copula_levels("t"))
    res = est.estimate_tail_dependence(probs=cc.PROBS, corr=cc.CORR, densities=_densities(_uniform_three()))
    z, dz = cc.off_diagonal(res.z), _diagonal_z(res, cc.PROBS)
    print(f"\nStudent-t copula end to end: z = {np.array2string(z, precision=4)}, diagonal {np.array2string(dz, precision=3)}")
    assert np.all(z[0] > cc.Z_T_BOUND)
    assert np.all(np.abs(dz) < cc.Z_BOUND)
    assert np.all(res.chi[0][np.triu_indices(3, 1)] > res.chi_model[0][np.triu_indices(3, 1)])


def test_lower_tail_mirrors_the_upper_and_both_stacks_them(hip):
    rng = np.random.default_rng(12)
    F = np.linalg.cholesky(cc.CORR)
    levels = []
    for l, n in enumerate((1000, 300)):
        zf = F @ rng.standard_normal((3, n))
        zc = None if l == 0 else zf + 0.2 * rng.standard_normal((3, n))
        levels.append((special.ndtr(zf), None if zc is None else special.ndtr(zc)))
    probs = (0.8, 0.9)
    near = min(np.min(np.abs(x - p)) for f, c in levels for x in (f, c) if x is not None for p in probs)
    assert near > 1e-9                                               # no sample within a rounding of a threshold
    dens = _densities(_uniform_three())
    est = _estimate(levels)
    up = est.estimate_tail_dependence(probs=probs, tail="upper", corr=cc.CORR, densities=dens)
    both = est.estimate_tail_dependence(probs=probs, tail="both", corr=cc.CORR, densities=dens)
    low = est.estimate_tail_dependence(probs=probs, tail="lower", corr=cc.CORR, densities=dens)
    assert both.prob.shape == (4, 3, 3)
    for name in ("prob", "var", "chi", "model", "chi_model", "z", "marginal"):
        assert np.array_equal(getattr(both, name), np.concatenate([getattr(up, name), getattr(low, name)]), equal_nan=True), name
    assert np.array_equal(both.counts.pair, np.concatenate([up.counts.pair, low.counts.pair], axis=1))
    assert np.array_equal(low.model, up.model)
    mirrored = _estimate([(1.0 - f, None if c is None else 1.0 - c) for f, c in levels])
    low_m = mirrored.estimate_tail_dependence(probs=probs, tail="lower", corr=cc.CORR, densities=dens)
    assert np.array_equal(low_m.counts.pair, up.counts.pair) and np.array_equal(low_m.prob, up.prob)
    assert np.array_equal(low_m.z, up.z, equal_nan=True)


def test_joint_frequency(gauss_estimate):
    levels = cc.copula_levels("gauss")
    lower = np.array([[0.85, 0.85, 0.85], [0.2, -INF, 0.5]])
    upper = np.array([[INF, INF, INF], [0.9, 0.7, INF]])
    res = gauss_estimate.estimate_joint_frequency(lower, upper)
    n, _, all_ = _twin_levels(levels, lower, upper)
    assert np.array_equal(res.counts.all, all_) and np.array_equal(res.n_samples, n) and res.counts.pair is None
    _, _, prob, var = cc.twin_level_statistics(n, all_)
    assert np.array_equal(res.prob, prob) and np.allclose(res.stderr, np.sqrt(var), rtol=1e-13, atol=0)
    assert res.prob.shape == (2,) and 0.02 < res.prob[0] < 0.05
    model, _ = gauss_estimate.estimate_joint_probability(lower, upper, corr=cc.CORR, densities=_densities(_uniform_three()))
    z = (res.prob - model.prob) / np.sqrt(res.stderr ** 2 + model.stderr ** 2)
    print(f"\njoint frequency {res.prob} +- {res.stderr}, model {model.prob} +- {model.stderr}")
    assert np.all(np.abs(res.prob - model.prob) <= 5.0 * res.stderr), z
    one = gauss_estimate.estimate_joint_frequency(lower[0], upper[0])
    assert one.prob.shape == (1,) and one.prob[0] == res.prob[0]
