"""GPU tests of the batched, seeded bootstrap (Estimate.est_bootstrap_batch, mlmc_bootstrap_*): the exported weights, every replicate
against estimate_mean over its explicit resample, determinism and the prefix property, the attributes of est_bootstrap, statistical
agreement with the loop, the storages, limits and errors, and bs_target_var_n_estimated(batch=True)."""
import collections
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


def _spec(M=1):
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    return [QuantitySpec(name="x", unit="m", shape=(M, 1), times=[1], locations=['0'])]


def _root_q(st, M=1):
    from mlmc_amd.quantity.quantity import make_root_quantity
    q = make_root_quantity(st, _spec(M))['x'][1]['0']
    return q[0, 0] if M == 1 else q


def _levels(N, M=1, seed=3, positive=False, nan=True, spread=1.0):
    rng = np.random.default_rng(seed)
    out = []
    for l, n in enumerate(N):
        f = spread * rng.normal(size=(M, n)) + 0.1 * np.arange(M)[:, None]
        c = None if l == 0 else f + 0.3 * 0.5 ** l * rng.normal(size=(M, n))
        if positive:
            f = np.exp(f)
            c = None if c is None else np.exp(c)
        if nan:
            f[0, 5::97] = np.nan
            if c is not None:
                c[M - 1, 11::193] = np.nan
        out.append((f, c))
    return out


def _memory(levels, M=1, chunk_size=None, n_ops=True):
    from mlmc_amd.sample_storage import Memory
    st = Memory(chunk_size=chunk_size)
    steps = [0.5 * 0.2 ** l for l in range(len(levels))]
    st.save_global_data(result_format=_spec(M), level_parameters=[[s] for s in steps])
    for l, (f, c) in enumerate(levels):
        st.set_level_samples(l, f.T, None if c is None else c.T)
    if n_ops:
        st.save_n_ops([(l, ((1 / h) ** 2 * len(levels[l][0][0]), len(levels[l][0][0]))) for l, h in enumerate(steps)])
    return st


def _resample_levels(q, st, k, seed, B, b):
    """The explicit resample of replicate b: every stored chunk's columns of q repeated by its exported weights, the chunks of a
    level concatenated -> [(fine [M, n'], coarse | None)] per level, and the weights per chunk."""
    from mlmc_amd import engine
    from mlmc_amd.quantity import quantity_estimate as qe
    N = [int(v) for v in st.get_n_collected()]
    L = len(N)
    parts = [[] for _ in range(L)]
    chunk_no = collections.Counter()
    for cs in q.get_quantity_storage().chunks():
        l = int(cs.level_id)
        c = chunk_no[l]
        chunk_no[l] += 1
        raw = np.asarray(q.samples(cs))
        raw = raw.reshape(-1, raw.shape[-2], raw.shape[-1])
        n = raw.shape[1]
        if n == 0:
            continue
        size = qe.bootstrap_sizes(seed, l, c, k[l], N[l], n, B)[b]
        w = engine.bootstrap_weights(n, [size], seed, qe.bootstrap_stream(l, c), b0=b)[0]
        assert w.sum() == size and w.min() >= 0
        parts[l].append(raw[:, np.repeat(np.arange(n), w), :])
    out = []
    for l in range(L):
        x = np.concatenate(parts[l], axis=1)
        out.append((x[:, :, 0], x[:, :, 1] if (l > 0 and x.shape[2] > 1) else None))
    return out


def _check_replicate(q, st, fn, k, seed, B, res, b, M=1):
    """Replicate b of `res` against estimate_mean(moments(q', fn, mom_at_bottom=False)) over its explicit resample q'."""
    from mlmc_amd.quantity import quantity_estimate as qe
    lv = _resample_levels(q, st, k, seed, B, b)
    st2 = _memory(lv, M, n_ops=False)
    qe.device_cache_clear()
    ref = qe.estimate_mean(qe.moments(_root_q(st2, M), fn, mom_at_bottom=False))
    assert np.array_equal(res.n_samples[b], ref.n_samples), (b, res.n_samples[b], ref.n_samples)
    # scales: sum |w d| and sum |w d^2| of the kept samples, per level and row (device rows -> 'on the surface' order)
    L, R = len(lv), fn.size
    for l, (f, c) in enumerate(lv):
        vf = fn.eval_all(f)                                        # [M, n, R], NaN where masked
        vc = fn.eval_all(c) if c is not None else np.zeros_like(vf)
        keep = ~np.any(np.isnan(vf), axis=(0, 2)) & ~np.any(np.isnan(vc), axis=(0, 2))
        d = (vf - vc)[:, keep, :]                                 # [M, n_kept, R]
        n_l = max(int(keep.sum()), 1)
        s1 = np.sum(np.abs(d), axis=1).T.reshape(-1)               # [R * M] in (moment, component) order
        s2 = np.sum(d * d, axis=1).T.reshape(-1)
        got_m = np.asarray(res.l_means[b][l]).reshape(-1)
        want_m = np.asarray(ref.l_means[l]).reshape(-1)
        got_v = np.asarray(res.l_vars[b][l]).reshape(-1)
        want_v = np.asarray(ref.l_vars[l]).reshape(-1)
        assert np.all(np.abs(got_m - want_m) <= 1e-12 * (s1 / n_l) + 1e-300), (b, l, np.max(np.abs(got_m - want_m)))
        if n_l > 1:
            tol_v = 1e-12 * (s2 + s1 * s1 / n_l) / (n_l - 1) + 1e-300
            assert np.all(np.abs(got_v - want_v) <= tol_v), (b, l, np.max(np.abs(got_v - want_v) / tol_v))
        else:
            assert np.all(np.isinf(got_v))
    assert L == res.n_samples.shape[1]


# ---- 1. weights ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,B", [(n, B) for n in (1, 7, 1000, 70001) for B in (1, 17, 300)] + [(3_000_000, 4)])
def test_weights_are_multinomial(hip, n, B):
    from mlmc_amd import engine
    rng = np.random.default_rng(n + B)
    sizes = rng.integers(0, n + 1, size=B)
    sizes[0] = n
    w = engine.bootstrap_weights(n, sizes, seed=12345, stream=7)
    assert w.shape == (B, n) and w.dtype == np.int32
    assert np.all(w >= 0)
    assert np.array_equal(w.sum(axis=1), sizes)                       # exact row sums
    # a replicate's row depends on (seed, stream, n, b, size) only
    if B > 1:
        assert np.array_equal(engine.bootstrap_weights(n, sizes[1:], seed=12345, stream=7, b0=1), w[1:])
    if n >= 1000:
        assert not np.array_equal(engine.bootstrap_weights(n, sizes[:1], seed=12345, stream=8), w[:1])
    total = int(sizes.sum())
    if n >= 64 and total >= 64 * 50:
        # uniform across the sample range (64 equal bins, tiles included) and inside the 4096-sample tiles
        col = w.sum(axis=0).astype(np.float64)
        edges = np.linspace(0, n, 65).astype(int)
        obs = np.add.reduceat(col, edges[:-1])
        exp = total * np.diff(edges) / n
        chi2 = np.sum((obs - exp) ** 2 / exp)
        assert chi2 < 63 + 6 * np.sqrt(2 * 63), chi2
        if n >= 4096:
            full = (n // 4096) * 4096
            inner = col[:full].reshape(-1, 64, 64).sum(axis=(0, 2))       # position inside the tile, 64 bins
            e = inner.sum() / 64
            chi2 = np.sum((inner - e) ** 2 / e)
            assert chi2 < 63 + 6 * np.sqrt(2 * 63), chi2
    if B >= 17 and n >= 7:
        # per-position mean / variance over replicates of one size s: Multinomial(s, 1 / n)
        s = n
        ws = engine.bootstrap_weights(n, np.full(B, s), seed=99, stream=1).astype(np.float64)
        p = 1.0 / n
        assert abs(ws.mean() - s * p) < 1e-12
        var = ws.var(axis=0, ddof=1).mean()
        want = s * p * (1 - p)
        assert abs(var - want) < 6 * want * np.sqrt(2.0 / (B - 1) / max(n, 1)) + 0.05 * want, (var, want)


# ---- 2. replicate == explicit resample ---------------------------------------------------------------------------------------------
def _fn_cases():
    from mlmc_amd import Legendre, Monomial, Fourier
    return {
        "leg1": (lambda: Legendre(1, (-2.0, 2.0)), False, 1),
        "leg6": (lambda: Legendre(6, (-2.0, 2.0)), False, 1),
        "leg64": (lambda: Legendre(64, (-2.5, 2.5)), False, 1),
        "leg128": (lambda: Legendre(128, (-2.5, 2.5)), False, 1),
        "mono": (lambda: Monomial(5, (-2.0, 2.0)), False, 1),
        "fourier": (lambda: Fourier(6, (-2.0, 2.0)), False, 1),
        "leglog": (lambda: Legendre(6, (0.2, 6.0), log=True), True, 1),
        "vector": (lambda: Legendre(8, (-2.0, 2.5)), False, 12),
    }


@pytest.mark.parametrize("case", list(_fn_cases()))
def test_replicate_equals_explicit_resample(hip, case):
    from mlmc_amd.estimator import Estimate
    make_fn, positive, M = _fn_cases()[case]
    fn = make_fn()
    N = [3000, 2400, 2100]                                   # three stored chunks per level
    st = _memory(_levels(N, M, seed=7, positive=positive), M, chunk_size=1000)
    q = _root_q(st, M)
    k = [1700, 900, 500]
    res = Estimate(q, st, fn).est_bootstrap_batch(300, sample_vector=k, seed=2024)
    assert res.seed == 2024 and res.n_samples.shape == (300, 3)
    for b in (0, 150, 299):
        _check_replicate(q, st, fn, k, 2024, 300, res, b, M)


# ---- 3. determinism and prefix ------------------------------------------------------------------------------------------------------
def test_bit_identical_runs_and_prefix(hip):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    st = _memory(_levels([5000, 2000, 700], 3, seed=4), 3, chunk_size=1500)
    q = _root_q(st, 3)
    est = Estimate(q, st, Legendre(10, (-2.0, 2.5)))
    a = est.est_bootstrap_batch(300, sample_vector=[2500, 1000, 300], seed=11)
    b = est.est_bootstrap_batch(300, sample_vector=[2500, 1000, 300], seed=11)
    c = est.est_bootstrap_batch(50, sample_vector=[2500, 1000, 300], seed=11)
    for name in ("n_samples", "l_means", "l_vars", "mean", "var"):
        x, y, z = getattr(a, name), getattr(b, name), getattr(c, name)
        assert np.array_equal(x, y, equal_nan=True), name
        assert np.array_equal(x[:50], z, equal_nan=True), name
    d = est.est_bootstrap_batch(300, sample_vector=[2500, 1000, 300], seed=12)
    assert not np.array_equal(a.l_means, d.l_means)
    # seed=None draws the seed from quantity.RNG: seeding that RNG makes the call reproducible
    from mlmc_amd.quantity import quantity as qmod
    qmod.RNG = np.random.default_rng(5)
    e1 = est.est_bootstrap_batch(20)
    qmod.RNG = np.random.default_rng(5)
    e2 = est.est_bootstrap_batch(20)
    assert e1.seed == e2.seed and np.array_equal(e1.l_means, e2.l_means)


# ---- 4. attributes --------------------------------------------------------------------------------------------------------------------
ATTRS = ("mean_bs_mean", "mean_bs_var", "mean_bs_l_means", "mean_bs_l_vars", "var_bs_mean", "var_bs_var", "var_bs_l_means",
         "var_bs_l_vars", "_bs_level_mean_variance")


@pytest.mark.parametrize("M", [1, 4])
def test_attributes_match_est_bootstrap(hip, M):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    st = _memory(_levels([2000, 800, 300], M, seed=9), M, chunk_size=700)
    q = _root_q(st, M)
    loop = Estimate(q, st, Legendre(5, (-2.0, 2.5)))
    loop.est_bootstrap(n_subsamples=5, sample_vector=[500, 200, 100])
    batch = Estimate(q, st, Legendre(5, (-2.0, 2.5)))
    r = batch.est_bootstrap_batch(40, sample_vector=[500, 200, 100], seed=3)
    for name in ATTRS:
        assert np.shape(getattr(batch, name)) == np.shape(getattr(loop, name)), name
    assert np.array_equal(batch.mean_bs_mean, np.mean(r.mean, axis=0))
    assert np.array_equal(batch.var_bs_var, np.var(r.var, axis=0, ddof=1))
    assert np.array_equal(batch.mean_bs_l_vars, np.mean(r.l_vars, axis=0))
    assert np.array_equal(batch.var_bs_l_means, np.var(r.l_means, axis=0, ddof=1))
    n_coll = np.array(st.get_n_collected())
    assert np.array_equal(batch._bs_level_mean_variance,
                          batch.var_bs_l_means * n_coll.reshape((-1,) + (1,) * (batch.var_bs_l_means.ndim - 1)))
    assert r.mean.shape == (40,) + np.shape(loop.mean_bs_mean) and r.l_means.shape == (40,) + np.shape(loop.mean_bs_l_means)


# ---- 5. statistical agreement with the loop -----------------------------------------------------------------------------------------
def test_statistical_agreement_with_the_loop(hip):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity as qmod
    st = _memory(_levels([2000, 800, 300], 1, seed=21, nan=False, spread=0.5), 1, chunk_size=600)
    q = _root_q(st, 1)
    k = [400, 150, 60]
    qmod.RNG = np.random.default_rng(77)
    loop = Estimate(q, st, Legendre(4, (-3.0, 3.0)))
    loop.est_bootstrap(n_subsamples=400, sample_vector=k)
    batch = Estimate(q, st, Legendre(4, (-3.0, 3.0)))
    r = batch.est_bootstrap_batch(400, sample_vector=k, seed=78)
    B = 400
    z = (batch.mean_bs_mean[1:] - loop.mean_bs_mean[1:]) / np.sqrt((batch.var_bs_mean[1:] + loop.var_bs_mean[1:]) / B)
    assert np.all(np.abs(z) < 5), z
    z = (batch.mean_bs_var[1:] - loop.mean_bs_var[1:]) / np.sqrt((batch.var_bs_var[1:] + loop.var_bs_var[1:]) / B)
    assert np.all(np.abs(z) < 5), z
    ratio = batch.var_bs_mean[1:] / loop.var_bs_mean[1:]
    assert np.all(np.abs(np.log(ratio)) < 5 * np.sqrt(2 * 2.0 / (B - 1))), ratio
    mean_sizes = r.n_samples.mean(axis=0)
    sd = np.sqrt(np.var(r.n_samples, axis=0, ddof=1) / B) + 1e-9
    assert np.all(np.abs(mean_sizes - np.array(k)) < 5 * sd + 0.5), (mean_sizes, k)


# ---- 6. storages -----------------------------------------------------------------------------------------------------------------------
def test_device_memory_storage(hip):
    import torch
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.sample_storage import DeviceMemory
    levels = _levels([3000, 900, 400], 2, seed=31)
    dev = DeviceMemory()
    dev.save_global_data(result_format=_spec(2), level_parameters=[[0.5], [0.1], [0.02]])
    for l, (f, c) in enumerate(levels):
        pairs = np.stack([f, np.zeros_like(f) if c is None else c], axis=-1)
        dev.set_level_samples(l, torch.from_numpy(pairs).cuda())
    qe.device_cache_clear()
    fn = Legendre(6, (-2.0, 2.5))
    q = _root_q(dev, 2)
    res = Estimate(q, dev, fn).est_bootstrap_batch(60, sample_vector=[1000, 500, 400], seed=8)
    host = _memory([(f, np.zeros_like(f) if c is None else c) for f, c in levels], 2, n_ops=False)
    # the same samples in a host storage (one chunk per level) give the same replicates
    ref = Estimate(_root_q(host, 2), host, fn).est_bootstrap_batch(60, sample_vector=[1000, 500, 400], seed=8)
    assert np.array_equal(res.n_samples, ref.n_samples)
    assert np.allclose(res.l_means, ref.l_means, rtol=1e-12, atol=1e-14)
    _check_replicate(_root_q(host, 2), host, fn, [1000, 500, 400], 8, 60, res, 59, 2)


def test_synth_device_storage(hip):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.sim.synth_device import SynthDeviceStorage
    st = SynthDeviceStorage([[0.5], [0.1], [0.02]], [4000, 1500, 600], chunk_size=1024)
    q = make_root_quantity(st, st.load_result_format())['length'][1]['10'][0]
    qe.device_cache_clear()
    fn = Legendre(5, (0.0, 6.0))
    k = [2000, 700, 300]
    res = Estimate(q, st, fn).est_bootstrap_batch(40, sample_vector=k, seed=5)
    assert res.n_samples.shape == (40, 3) and np.all(np.isfinite(res.mean))
    # the explicit resample of the host view of the same samples
    lv = _resample_levels(q, st, k, 5, 40, 17)
    st2 = _memory(lv, 1, n_ops=False)
    ref = qe.estimate_mean(qe.moments(_root_q(st2, 1), fn, mom_at_bottom=False))
    assert np.array_equal(res.n_samples[17], ref.n_samples)
    assert np.allclose(res.l_means[17], ref.l_means, rtol=1e-11, atol=1e-13)
    assert np.allclose(res.l_vars[17], ref.l_vars, rtol=1e-10, atol=1e-13)


@pytest.mark.parametrize("device_tree", ["1", "0"])
def test_derived_quantity_and_host_tree(hip, device_tree):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    st = _memory(_levels([2500, 900, 400], 1, seed=41), 1, chunk_size=800)
    fn = Legendre(6, (0.0, 4.0))
    k = [1200, 600, 200]
    os.environ["MLMC_HIP_DEVICE_TREE"] = device_tree
    try:
        qe.device_cache_clear()
        q0 = _root_q(st, 1)
        q = (q0 - 0.5) * (q0 - 0.5)
        res = Estimate(q, st, fn).est_bootstrap_batch(50, sample_vector=k, seed=6)
        for b in (0, 49):
            lv = _resample_levels(q, st, k, 6, 50, b)
            ref = qe.estimate_mean(qe.moments(_root_q(_memory(lv, 1, n_ops=False), 1), fn, mom_at_bottom=False))
            assert np.array_equal(res.n_samples[b], ref.n_samples)
            assert np.allclose(res.l_means[b], ref.l_means, rtol=1e-11, atol=1e-13)
            assert np.allclose(res.l_vars[b], ref.l_vars, rtol=1e-10, atol=1e-13)
    finally:
        os.environ.pop("MLMC_HIP_DEVICE_TREE", None)
        qe.device_cache_clear()


# ---- 7. limits and errors --------------------------------------------------------------------------------------------------------------
def test_zero_requested_samples_at_a_level(hip):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    st = _memory(_levels([1500, 600, 300], 1, seed=51), 1, chunk_size=500)
    q = _root_q(st, 1)
    loop = Estimate(q, st, Legendre(4, (-2.0, 2.0)))
    loop.est_bootstrap(n_subsamples=3, sample_vector=[600, 0, 300])
    r = Estimate(q, st, Legendre(4, (-2.0, 2.0))).est_bootstrap_batch(30, sample_vector=[600, 0, 300], seed=1)
    assert np.all(r.n_samples[:, 1] == 0)
    assert np.all(np.isnan(r.l_means[:, 1])) and np.all(np.isinf(r.l_vars[:, 1]))
    assert np.all(np.isnan(loop.mean_bs_l_means[1])) and np.all(np.isinf(loop.mean_bs_l_vars[1]))
    assert np.all(np.isnan(r.mean)) and np.all(np.isnan(loop.mean_bs_mean))
    # k_l = N_l: every chunk gives all its samples' worth of picks
    r = Estimate(q, st, Legendre(4, (-2.0, 2.0))).est_bootstrap_batch(10, sample_vector=[1500, 600, 300], seed=1)
    assert np.all(r.n_samples <= np.array([1500, 600, 300])) and np.all(r.n_samples > 0)


def test_all_samples_masked(hip):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    st = _memory(_levels([500, 200], 1, seed=61), 1)
    q = _root_q(st, 1)
    with pytest.raises(Exception, match="All samples were masked"):
        Estimate(q, st, Legendre(4, (100.0, 101.0))).est_bootstrap(n_subsamples=2)
    with pytest.raises(Exception, match="All samples were masked"):
        Estimate(q, st, Legendre(4, (100.0, 101.0))).est_bootstrap_batch(5, seed=2)


def test_unsupported_moments_raise(hip):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.moments import Spline, TransformedMoments
    st = _memory(_levels([500, 200], 1, seed=62), 1)
    est = Estimate(_root_q(st, 1), st, Legendre(4, (-2.0, 2.0)))
    for fn in (Spline(6, (-2.0, 2.0)), TransformedMoments(Legendre(4, (-2.0, 2.0)), np.eye(3, 4))):
        with pytest.raises(ValueError, match="est_bootstrap"):
            est.est_bootstrap_batch(5, moments_fn=fn, seed=1)


def test_ten_thousand_replicates_run_in_groups(hip):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    st = _memory(_levels([3000, 1000, 400], 1, seed=71), 1, chunk_size=1000)
    est = Estimate(_root_q(st, 1), st, Legendre(6, (-2.0, 2.5)))
    big = est.est_bootstrap_batch(10_000, sample_vector=[1000, 500, 200], seed=13)
    small = est.est_bootstrap_batch(300, sample_vector=[1000, 500, 200], seed=13)
    assert big.n_samples.shape == (10_000, 3)
    assert np.array_equal(big.l_means[:300], small.l_means) and np.array_equal(big.l_vars[:300], small.l_vars)
    assert np.all(big.n_samples.sum(axis=1) > 0)


def test_ten_million_sample_level(hip):
    from mlmc_amd import Legendre, engine
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    n = 10_000_000
    rng = np.random.default_rng(81)
    f = rng.normal(size=(1, n))
    st = _memory([(f, None)], 1, n_ops=False)
    fn = Legendre(64, (-6.0, 6.0))
    k = [7_000_000]
    res = Estimate(_root_q(st, 1), st, fn).est_bootstrap_batch(300, sample_vector=k, seed=21)
    sizes = qe.bootstrap_sizes(21, 0, 0, k[0], n, n, 300)
    assert np.array_equal(res.n_samples[:, 0], sizes)                # every sample is kept: the counts are the sizes
    b = 123
    w = engine.bootstrap_weights(n, [sizes[b]], 21, qe.bootstrap_stream(0, 0), b0=b)[0]
    assert w.sum() == sizes[b]
    x = np.repeat(f[0], w)
    st2 = _memory([(x[None, :], None)], 1, n_ops=False)
    qe.device_cache_clear()
    ref = qe.estimate_mean(qe.moments(_root_q(st2, 1), fn, mom_at_bottom=False))
    assert np.array_equal(res.n_samples[b], ref.n_samples)
    vf = fn.eval_all(x[None, :])[0]
    s1 = np.sum(np.abs(vf), axis=0)
    s2 = np.sum(vf * vf, axis=0)
    m = len(x)
    assert np.all(np.abs(res.l_means[b][0] - ref.l_means[0]) <= 1e-12 * s1 / m)
    assert np.all(np.abs(res.l_vars[b][0] - ref.l_vars[0]) <= 1e-12 * (s2 + s1 * s1 / m) / (m - 1))


# ---- 8. bs_target_var_n_estimated(batch=True) --------------------------------------------------------------------------------------
def test_bs_target_var_n_estimated_batch(hip):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate, estimate_n_samples_for_target_variance
    st = _memory(_levels([3000, 1200, 500], 1, seed=91, nan=False), 1, chunk_size=1000)
    q = _root_q(st, 1)
    fn = Legendre(5, (-3.0, 3.0))
    got = Estimate(q, st, fn).bs_target_var_n_estimated(1e-4, batch=True, seed=17)
    est = Estimate(q, st, fn)
    est.est_bootstrap_batch(300, seed=17)
    variances, n_ops = est.estimate_diff_vars_regression(np.array(st.get_n_collected()), raw_vars=est.mean_bs_l_vars)
    want = estimate_n_samples_for_target_variance(1e-4, variances, n_ops, n_levels=3)
    assert np.array_equal(got, want)
