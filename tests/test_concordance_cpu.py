"""CPU tests of the concordance counts: the NumPy twin of mlmc_concordance_counts against a triple loop, the level statistics from
the integers against np.var of the explicit differences, tool.simple_distribution.bivariate_orthant against SciPy, the argument
errors that need no device, and the two copula cases of tests/concordance_cases.py on the twin alone."""
import numpy as np
import pytest
from scipy import special, stats

from tests import concordance_cases as cc


def _loop_counts(fine, coarse, lower, upper):
    """the definition column by column"""
    M, n = fine.shape
    G = lower.shape[0]
    pair = np.zeros((G, 3, M, M), dtype=np.int64)
    all_ = np.zeros((G, 3), dtype=np.int64)
    kept = 0
    for j in range(n):
        if any(np.isnan(fine[m, j]) or (coarse is not None and np.isnan(coarse[m, j])) for m in range(M)):
            continue
        kept += 1
        for g in range(G):
            ef = [bool(lower[g, m] < fine[m, j] and fine[m, j] < upper[g, m]) for m in range(M)]
            ec = [bool(coarse is not None and lower[g, m] < coarse[m, j] and coarse[m, j] < upper[g, m]) for m in range(M)]
            for a in range(M):
                for b in range(M):
                    jf, jc = ef[a] and ef[b], ec[a] and ec[b]
                    pair[g, 0, a, b] += jf
                    pair[g, 1, a, b] += jc
                    pair[g, 2, a, b] += jf != jc
            af, ac = all(ef), all(ec) and coarse is not None
            all_[g] += (af, ac, af != ac)
    return pair, all_, kept


@pytest.mark.parametrize("with_coarse", [False, True])
def test_twin_against_the_triple_loop(with_coarse):
    rng = np.random.default_rng(5)
    M, n = 4, 37
    fine = rng.integers(-2, 3, size=(M, n)).astype(np.float64)          # small integers: many values exactly on a limit
    coarse = fine + rng.integers(-1, 2, size=(M, n)) if with_coarse else None
    fine[1, 3] = np.nan
    fine[2, 9] = np.inf
    fine[0, 11] = -np.inf
    if with_coarse:
        coarse[3, 20] = np.nan
    lower = np.array([[-1.0, -np.inf, 0.0, -1.0], [-np.inf] * 4, [0.0, 0.0, 0.0, 0.0]])
    upper = np.array([[2.0, 1.0, np.inf, 1.0], [np.inf] * 4, [np.inf, 2.0, 1.0, np.inf]])
    pair, all_, kept = cc.twin_counts(fine, coarse, lower, upper)
    ref = _loop_counts(fine, coarse, lower, upper)
    assert np.array_equal(pair, ref[0]) and np.array_equal(all_, ref[1]) and kept == ref[2]
    assert kept == n - (2 if with_coarse else 1)
    assert np.array_equal(pair, pair.transpose(0, 1, 3, 2))
    # the unbounded event: every kept column with finite or infinite values is inside, unless a value IS an infinity (open box)
    assert all_[1, 0] == kept - 2
    if not with_coarse:
        assert np.all(pair[:, 1] == 0) and np.array_equal(pair[:, 2], pair[:, 0]) and np.all(all_[:, 1] == 0)


def test_level_statistics_against_explicit_differences():
    rng = np.random.default_rng(6)
    M = 3
    lower, upper = np.array([[0.2] * M, [0.6] * M]), np.full((2, M), np.inf)
    levels, counts = [], []
    for l, n in enumerate((200, 57, 1)):
        f = rng.uniform(size=(M, n))
        c = None if l == 0 else np.clip(f + 0.1 * rng.standard_normal((M, n)), 0.0, 1.0)
        levels.append((f, c))
        counts.append(cc.twin_counts(f, c, lower, upper))
    n = np.array([c[2] for c in counts])
    l_means, l_vars, prob, var = cc.twin_level_statistics(n, np.array([c[0] for c in counts]))
    for l, (f, c) in enumerate(levels):
        for g in range(2):
            for a in range(M):
                for b in range(M):
                    d = ((f[a] > lower[g, a]) & (f[b] > lower[g, b])).astype(np.float64)
                    if c is not None:
                        d -= ((c[a] > lower[g, a]) & (c[b] > lower[g, b])).astype(np.float64)
                    assert set(np.unique(d)) <= {-1.0, 0.0, 1.0}
                    assert abs(l_means[l, g, a, b] - d.mean()) <= 1e-15
                    if d.size > 1:
                        assert abs(l_vars[l, g, a, b] - np.var(d, ddof=1)) <= 1e-14
                    else:
                        assert l_vars[l, g, a, b] == np.inf
    assert np.all(np.isinf(var))                                    # the level with one sample
    assert np.allclose(prob, l_means.sum(axis=0), rtol=0, atol=1e-15)
    # the product's statistics are the twin's
    from mlmc_amd.quantity import quantity_estimate as qe
    st = qe.concordance_statistics(n, np.array([c[0] for c in counts]))
    assert np.array_equal(st["l_means"], l_means) and np.array_equal(st["l_vars"], l_vars)
    assert np.array_equal(st["prob"], prob) and np.array_equal(st["var"], var)
    st_all = qe.concordance_statistics(n[:2], np.array([c[1] for c in counts[:2]]))
    ref_all = cc.twin_level_statistics(n[:2], np.array([c[1] for c in counts[:2]]))
    assert st_all["prob"].shape == (2,) and np.array_equal(st_all["prob"], ref_all[2])
    assert np.allclose(st_all["var"], ref_all[3], rtol=1e-14, atol=0)


def test_bivariate_orthant():
    from mlmc_amd.tool import simple_distribution as sd
    worst = 0.0
    for rho in (0.0, 0.3, 0.6, -0.5, 0.95, 0.999):
        for p in (0.9, 0.99):
            h = special.ndtri(p)
            ref = stats.multivariate_normal.cdf([-h, -h], mean=[0.0, 0.0], cov=[[1.0, rho], [rho, 1.0]])
            got = sd.bivariate_orthant(h, h, rho)
            worst = max(worst, abs(got - ref))
            assert abs(got - ref) <= 1e-15 + 1e-13 * ref, (rho, p, got, ref)       # SciPy's own integration is not exact either
            assert abs(sd.bivariate_orthant(h, h, rho, nodes=32) - got) <= 1e-15
    print(f"\nbivariate_orthant against scipy: worst absolute difference {worst:.3g}")
    h, k = np.array([-1.5, 0.0, 0.7, 2.5])[:, None], np.array([-0.3, 1.1, 3.0])[None, :]
    # rho = 0: the product; the symmetry (h, k) <-> (k, h); the limits rho = 1, -1
    assert np.allclose(sd.bivariate_orthant(h, k, 0.0), special.ndtr(-h) * special.ndtr(-k), rtol=1e-15, atol=0)
    for rho in (0.4, -0.7, 0.999):
        assert np.allclose(sd.bivariate_orthant(h, k, rho), sd.bivariate_orthant(k, h, rho), rtol=1e-14, atol=1e-18)
        ref = np.array([[stats.multivariate_normal.cdf([-a, -b], mean=[0.0, 0.0], cov=[[1.0, rho], [rho, 1.0]]) for b in k[0]]
                        for a in h[:, 0]])
        assert np.allclose(sd.bivariate_orthant(h, k, rho), ref, rtol=1e-9, atol=1e-14)
    assert np.array_equal(sd.bivariate_orthant(h, k, 1.0), special.ndtr(-np.maximum(h, k)) + 0 * h)
    assert np.array_equal(sd.bivariate_orthant(h, k, -1.0), np.maximum(0.0, special.ndtr(-k) - special.ndtr(h)))
    # continuity into the limits
    assert np.allclose(sd.bivariate_orthant(h, k, 1.0 - 1e-12), sd.bivariate_orthant(h, k, 1.0), rtol=0, atol=1e-6)
    assert np.allclose(sd.bivariate_orthant(h, k, -1.0 + 1e-12), sd.bivariate_orthant(h, k, -1.0), rtol=0, atol=1e-6)
    mixed = sd.bivariate_orthant(1.0, 0.5, np.array([0.3, 1.0, -1.0]))
    assert mixed.shape == (3,) and mixed[1] == special.ndtr(-1.0) and mixed[2] == 0.0
    assert isinstance(sd.bivariate_orthant(0.0, 0.0, 0.0), float) and sd.bivariate_orthant(0.0, 0.0, 0.0) == 0.25
    with pytest.raises(ValueError, match="rho"):
        sd.bivariate_orthant(0.0, 0.0, 1.5)
    with pytest.raises(ValueError, match="rho"):
        sd.bivariate_orthant(0.0, 0.0, np.nan)


def test_argument_errors_without_a_device():
    from mlmc_amd.tool import simple_distribution as sd
    x = np.zeros((3, 8))
    with pytest.raises(ValueError, match=r"must be \[M, n\]"):
        sd.concordance_counts(np.zeros(8), lower=0.0, upper=1.0)
    with pytest.raises(ValueError, match="differ in shape"):
        sd.concordance_counts(x, np.zeros((3, 7)), lower=0.0, upper=1.0)
    with pytest.raises(ValueError, match="NaN"):
        sd.concordance_counts(x, lower=[0.0, np.nan, 0.0], upper=1.0)
    with pytest.raises(ValueError, match="NaN"):
        sd.concordance_counts(x, lower=0.0, upper=np.nan)
    with pytest.raises(ValueError, match="broadcast"):
        sd.concordance_counts(x, lower=np.zeros((2, 4)), upper=1.0)
    with pytest.raises(ValueError, match="broadcast"):
        sd.concordance_counts(x, lower=np.zeros((2, 3)), upper=np.ones((3, 3)))
    with pytest.raises(ValueError, match="17 events"):
        sd.concordance_counts(x, lower=np.zeros((17, 3)), upper=1.0)
    with pytest.raises(ValueError, match="1025 components"):
        sd.concordance_counts(np.zeros((1025, 2)), lower=0.0, upper=1.0)
    import torch
    with pytest.raises(ValueError, match="float64 device tensor"):
        sd.concordance_counts(torch.zeros((3, 8), dtype=torch.float64), lower=0.0, upper=1.0)


def test_copula_cases_on_the_twin():
    """the Gaussian copula passes (|z| < 5 off the diagonal, the diagonal within 5 standard errors of 1 - p), the Student-t copula
    with the same correlations is found at p = 0.9 (every z > 8); the observed values are those the case file records"""
    p = np.array(cc.PROBS)
    prob, var, z = cc.twin_tail_z(cc.copula_levels("gauss"))
    zg = cc.off_diagonal(z)
    diag = np.array([(np.diag(pr) - (1.0 - pg)) / np.sqrt(np.diag(v)) for pr, v, pg in zip(prob, var, p)])
    print(f"\nGaussian copula: z = {np.array2string(zg, precision=4)}, diagonal {np.array2string(diag, precision=3)}")
    assert np.all(np.abs(zg) < cc.Z_BOUND) and np.all(np.abs(diag) < cc.Z_BOUND)
    assert np.allclose(zg, cc.Z_GAUSS, rtol=0, atol=1e-3)
    prob, var, z = cc.twin_tail_z(cc.copula_levels("t"))
    zt = cc.off_diagonal(z)
    diag = np.array([(np.diag(pr) - (1.0 - pg)) / np.sqrt(np.diag(v)) for pr, v, pg in zip(prob, var, p)])
    print(f"Student-t copula: z = {np.array2string(zt, precision=4)}, diagonal {np.array2string(diag, precision=3)}")
    assert np.all(zt[0] > cc.Z_T_BOUND)
    assert np.all(np.abs(diag) < cc.Z_BOUND)                        # its marginals are uniform all the same
    assert np.allclose(zt, cc.Z_T, rtol=0, atol=1e-3)
