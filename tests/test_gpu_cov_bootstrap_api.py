"""GPU tests of the covariance bootstrap through Estimate: est_bootstrap_component_covariance against the host recomputation from the
exported weights (the walk of the batched-bootstrap tests: bootstrap_sizes, bootstrap_stream, mlmc_bootstrap_weights; the long-double
sums of tests/xcov_boot_cases.py, their tolerance pushed through the finish), the counts against est_bootstrap_batch, the normal-score
route against normal_scores on the same chunks, the correlation bands, and the joint-exceedance bands replicate by replicate.
Storage: 3 levels, M = 3, Memory of (300, 120, 40) samples in chunks of 150 -- two chunks on level 0."""
import collections

import numpy as np
import pytest

from tests import xcov_boot_cases as xc
from tests.test_gpu_bootstrap_batch import _memory, _root_q

pytestmark = pytest.mark.gpu

N = [300, 120, 40]
K_REQ = [200, 90, 40]
M = 3
B = 16
SEED = 5
U = 2.0 ** -53


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


def _levels():
    """correlated near-normal components; a NaN in a fine and in a coarse value"""
    rng = np.random.default_rng(41)
    mix = np.array([[1.0, 0.0, 0.0], [0.6, 0.8, 0.0], [-0.3, 0.4, 0.86]])
    out = []
    for l, n in enumerate(N):
        f = mix @ rng.normal(size=(M, n)) + np.array([[0.5], [-0.2], [1.0]])
        c = None if l == 0 else f + 0.2 * 0.5 ** l * rng.normal(size=(M, n))
        out.append((f, c))
    out[0][0][1, 17] = np.nan
    out[1][1][2, 5] = np.nan
    return out


@pytest.fixture(scope="module")
def case(hip):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    st = _memory(_levels(), M, chunk_size=150)
    q = _root_q(st, M)
    est = Estimate(q, st, Legendre(5, (-6.0, 6.0)))
    return st, q, est


def _replicate_sums(q, st, shift, transform=None):
    """the level sums of every replicate in long double from the exported weights: n [B, L], s1, U1 [B, L, M], s2, U2 [B, L, M, M]"""
    from mlmc_amd import engine
    from mlmc_amd.quantity import quantity_estimate as qe
    L = len(N)
    n_r = np.zeros((B, L), dtype=np.int64)
    s1, U1 = (np.zeros((B, L, M), dtype=xc.LD) for _ in range(2))
    s2, U2 = (np.zeros((B, L, M, M), dtype=xc.LD) for _ in range(2))
    chunk_no = collections.Counter()
    for cs in q.get_quantity_storage().chunks():
        l = int(cs.level_id)
        c = chunk_no[l]
        chunk_no[l] += 1
        raw = np.asarray(q.samples(cs))
        raw = raw.reshape(-1, raw.shape[-2], raw.shape[-1])
        n = raw.shape[1]
        fine, coarse = raw[:, :, 0], (raw[:, :, 1] if l > 0 else None)
        if transform is not None:
            fine, coarse = transform(fine, coarse)
        sizes = qe.bootstrap_sizes(SEED, l, c, K_REQ[l], N[l], n, B)
        w = engine.bootstrap_weights(n, sizes, SEED, qe.bootstrap_stream(l, c)).astype(np.int64)
        got = xc.weighted_sums(fine, coarse, shift, w)
        n_r[:, l] += got[0]
        for dst, src in zip((s1, s2, U1, U2), got[1:]):
            dst[:, l] += src
    assert chunk_no[0] == 2 and chunk_no[1] == 1
    return n_r, s1, s2, U1, U2


def _check_finish(res, sums, shift):
    """mean, cov and corr of the call against the finish of the reference sums, within the tolerance of the level sums pushed
    through the finish: d m = sum_l t1 u U1 / n, d S = sum_l t2 u U2 / n, d cov = d S + |m_i| d m_j + |m_j| d m_i, d corr by the
    quotient rule, each plus a few roundings of the finish's own arithmetic"""
    from mlmc_amd.estimator import covariance_replicates
    n_r, s1, s2, U1, U2 = sums
    assert np.array_equal(res.n_samples, n_r)
    mean, cov, corr, ok = covariance_replicates(n_r, s1.astype(np.float64), s2.astype(np.float64), K_REQ, shift)
    assert ok.all() and np.array_equal(res.ok, ok)
    nf = n_r.astype(np.float64)
    t1 = np.array([xc.tolerance("level0" if l == 0 else "pair", "s1") for l in range(len(N))])
    t2 = np.array([xc.tolerance("level0" if l == 0 else "pair", "s2") for l in range(len(N))])
    U1f, U2f = U1.astype(np.float64), U2.astype(np.float64)
    dm = np.sum(t1[None, :, None] * U * U1f / nf[:, :, None], axis=1)
    dS = np.sum(t2[None, :, None, None] * U * U2f / nf[:, :, None, None], axis=1)
    a = np.zeros(M) if shift is None else shift
    m = mean - a
    eps = 2.0 ** -52
    round_m = 8 * eps * (np.sum(U1f / nf[:, :, None], axis=1) + np.abs(a))
    round_S = 8 * eps * (np.sum(U2f / nf[:, :, None, None], axis=1) + np.abs(m[:, :, None] * m[:, None, :]))
    dcov = dS + np.abs(m)[:, :, None] * dm[:, None, :] + np.abs(m)[:, None, :] * dm[:, :, None] + round_S
    var = np.diagonal(cov, axis1=1, axis2=2)
    dvar = np.diagonal(dcov, axis1=1, axis2=2)
    sd = np.sqrt(var)
    dcorr = dcov / (sd[:, :, None] * sd[:, None, :]) + np.abs(corr) * 0.5 * (dvar / var)[:, :, None] + \
        np.abs(corr) * 0.5 * (dvar / var)[:, None, :] + 8 * eps
    for name, got, want, tol in (("mean", res.mean, mean, dm + round_m), ("cov", res.cov, cov, dcov), ("corr", res.corr, corr, dcorr)):
        err = np.abs(got - want)
        print("{:4s} worst error / tolerance {:.3g}   (largest tolerance {:.3g})".format(name, float(np.max(err / tol)), float(tol.max())))
        assert np.all(err <= tol), (name, float(np.max(err / tol)))
    assert np.array_equal(res.cov, res.cov.transpose(0, 2, 1)) and np.array_equal(res.corr, res.corr.transpose(0, 2, 1))
    assert np.all(np.diagonal(res.corr, axis1=1, axis2=2) == 1.0)


def test_replicates_equal_the_host_recomputation_from_exported_weights(case):
    from mlmc_amd.quantity import quantity_estimate as qe
    st, q, est = case
    res = est.est_bootstrap_component_covariance(B, sample_vector=K_REQ, seed=SEED)
    assert res.seed == SEED and res.n_samples.shape == (B, 3) and res.mean.shape == (B, M) and res.cov.shape == res.corr.shape == (B, M, M)
    shift = np.asarray(qe.estimate_mean(q).mean, dtype=np.float64).reshape(M)
    _check_finish(res, _replicate_sums(q, st, shift), shift)
    again = est.est_bootstrap_component_covariance(B, sample_vector=K_REQ, seed=SEED)          # the pooled accumulator, reset
    for name in ("n_samples", "mean", "cov", "corr", "ok"):
        assert np.array_equal(getattr(res, name), getattr(again, name)), name
    longer = est.est_bootstrap_component_covariance(B + 9, sample_vector=K_REQ, seed=SEED)      # the prefix property
    assert np.array_equal(longer.corr[:B], res.corr) and np.array_equal(longer.n_samples[:B], res.n_samples)
    # raw second moments: no shift, `cov` = S_b
    raw = est.est_bootstrap_component_covariance(B, sample_vector=K_REQ, seed=SEED, centered=False)
    n_r, s1, s2, U1, U2 = _replicate_sums(q, st, None)
    S = np.sum(s2.astype(np.float64) / n_r[:, :, None, None], axis=1)
    tol = np.sum(xc.tolerance("level0", "s2") * U * U2.astype(np.float64) / n_r[:, :, None, None], axis=1) + 2.0 ** -49 * np.abs(S)
    assert np.all(np.abs(raw.cov - S) <= tol)
    assert np.allclose(raw.corr, res.corr, rtol=0, atol=1e-12)


def test_counts_equal_those_of_the_batched_moment_bootstrap(case):
    """the same streams and weights: with a moments domain that covers every sample, est_bootstrap_batch on the vector quantity keeps
    exactly the samples without a NaN"""
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    st, q, est = case
    res = est.est_bootstrap_component_covariance(B, sample_vector=K_REQ, seed=SEED)
    ref = Estimate(q, st, Legendre(3, (-50.0, 50.0))).est_bootstrap_batch(B, sample_vector=K_REQ, seed=SEED)
    assert np.array_equal(res.n_samples, ref.n_samples)
    assert res.n_samples[:, 1].max() == K_REQ[1] and res.n_samples[:, 1].min() < K_REQ[1]      # one chunk: K_REQ picks; the NaN was picked


def test_score_route_matches_normal_scores_on_the_same_chunks(case):
    from mlmc_amd.tool import simple_distribution as sd
    st, q, est = case
    dens = est.construct_densities()
    distrs = [d[0] for d in dens]

    def scores(fine, coarse):
        if coarse is None:
            return np.asarray(sd.normal_scores(distrs, fine)), None
        zf, zc = sd.normal_scores(distrs, fine, coarse)
        return np.asarray(zf), np.asarray(zc)
    res = est.est_bootstrap_component_covariance(B, sample_vector=K_REQ, seed=SEED, corr="scores", densities=dens)
    _check_finish(res, _replicate_sums(q, st, None, transform=scores), None)
    built = est.est_bootstrap_component_covariance(B, sample_vector=K_REQ, seed=SEED, corr="scores")   # densities constructed here
    assert np.array_equal(built.corr, res.corr)


def test_correlation_bands(case):
    from mlmc_amd.estimator import quantile_bands
    st, q, est = case
    for corr in (None, "scores"):
        dens = est.construct_densities() if corr == "scores" else None
        bands = est.bootstrap_component_correlation(B, sample_vector=K_REQ, seed=SEED, level=0.8, corr=corr, densities=dens)
        reps = est.est_bootstrap_component_covariance(B, sample_vector=K_REQ, seed=SEED, corr=corr, densities=dens)
        assert bands.seed == SEED and np.array_equal(bands.replicates, reps.corr) and np.array_equal(bands.ok, reps.ok)
        assert bands.n_ok == int(reps.ok.sum()) == B
        assert np.array_equal(bands.corr, est._copula_correlation("test", corr, dens, 1e-8, 0.0, 1e-4, None)[0])
        assert np.all(np.diag(bands.corr) == 1.0) and np.all(np.diag(bands.lo) == 1.0) and np.all(np.diag(bands.hi) == 1.0)
        assert np.all(bands.lo <= bands.hi) and np.all(np.diag(bands.std) == 0.0) and np.all(bands.std >= 0.0)
        lo, hi = quantile_bands(reps.corr.reshape(B, 1, M * M), reps.ok[:, None], 0.8)
        assert np.array_equal(bands.lo, lo.reshape(M, M)) and np.array_equal(bands.hi, hi.reshape(M, M))
        assert np.array_equal(bands.std, np.std(reps.corr, axis=0, ddof=1))
        off = ~np.eye(M, dtype=bool)
        assert np.all(bands.hi[off] - bands.lo[off] > 0.0)                       # the resampling does move the correlations


def test_joint_exceedance_bands_replicate_by_replicate(case):
    from mlmc_amd.estimator import quantile_bands
    from mlmc_amd.tool import simple_distribution as sd
    st, q, est = case
    dens = est.construct_densities()
    distrs = [d[0] for d in dens]
    thresholds = np.array([[1.0, 0.5, -np.inf], [1.5, 0.8, 1.8]])
    nb, n, seeds = 8, 2 ** 10, (0, 1)
    reps = est.est_bootstrap_component_covariance(nb, sample_vector=K_REQ, seed=SEED)
    base = est.estimate_joint_exceedance(thresholds, n=n, seeds=seeds, densities=dens)[0]

    # marginals fixed: only the dependence is resampled
    fixed = est.bootstrap_joint_exceedance(thresholds, n_subsamples=nb, sample_vector=K_REQ, seed=SEED, n=n, seeds=seeds, densities=dens)
    assert fixed.seed == SEED and fixed.replicates.shape == (nb, 2) and fixed.n_ok == int(fixed.ok.sum())
    assert np.array_equal(fixed.prob, base.prob) and np.array_equal(fixed.stderr, base.stderr)
    assert np.array_equal(fixed.ok, reps.ok) and fixed.ok.all()
    for b in range(nb):
        want = sd.joint_probabilities(distrs, thresholds, np.inf, n, list(seeds), corr=reps.corr[b]).prob
        assert np.array_equal(fixed.replicates[b], want), b
    lo, hi = quantile_bands(fixed.replicates[:, None, :], fixed.ok[:, None], 0.9)
    assert np.array_equal(fixed.lo, lo[0]) and np.array_equal(fixed.hi, hi[0]) and np.all(fixed.lo <= fixed.hi)
    assert np.ptp(fixed.replicates[:, 1]) > 0.0

    # marginals resampled: the replicate densities of est_bootstrap_components with the same seed -- the same picks
    res = est.bootstrap_joint_exceedance(thresholds, n_subsamples=nb, sample_vector=K_REQ, seed=SEED, n=n, seeds=seeds, densities=dens,
                                         marginals="resampled")
    fns = [d[3]._base for d in dens]
    comp = est.est_bootstrap_components(nb, sample_vector=K_REQ, moments_fns=fns, seed=SEED)
    R = int(fns[0].size)
    want_ok = reps.ok.copy()
    want = np.full((nb, 2), np.nan)
    for b in range(nb):
        d_b = []
        for m in range(M):
            mobj = dens[m][3]
            mu = np.sum([comp.l_means[b, l, m, :R] @ mobj._base_matrix.T for l in range(3)], axis=0)
            d_b.append(sd.SimpleDistribution(mobj, np.stack((mu, np.ones(mobj.size)), axis=1), domain=mobj.domain))
        results = sd.estimate_densities_minimize(d_b, 1e-8, 0.0)
        want_ok[b] &= all(bool(r.success) for r in results)                      # every component is constrained by a box
        if want_ok[b]:
            want[b] = sd.joint_probabilities(d_b, thresholds, np.inf, n, list(seeds), corr=reps.corr[b]).prob
    print("resampled marginals: ok", want_ok.tolist())
    assert np.array_equal(res.ok, want_ok) and res.n_ok == int(want_ok.sum()) and res.n_ok >= 1
    assert np.array_equal(res.replicates, want, equal_nan=True)
    lo, hi = quantile_bands(res.replicates[:, None, :], res.ok[:, None], 0.9)
    assert np.array_equal(res.lo, lo[0]) and np.array_equal(res.hi, hi[0])
    assert np.array_equal(res.prob, base.prob)
    assert not np.array_equal(res.replicates, fixed.replicates)
