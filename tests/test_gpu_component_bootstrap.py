"""GPU tests of the per-component bootstrap (Estimate.est_bootstrap_components, mlmc_bootstrap_create_multi / _finalize_multi) and of
the bootstrap bands of the component quantiles (Estimate.bootstrap_component_quantiles): every component against the scalar
est_bootstrap_batch on scalar_component(q, m) with the bounds of its own replicate test, a planted mask, determinism and the prefix
property, the storages, the quantile bands step by step, and the errors of the device route."""
import os

import numpy as np
import pytest

from tests.test_gpu_bootstrap_batch import _levels, _memory, _spec, _root_q, _resample_levels

pytestmark = pytest.mark.gpu

N = [3000, 2400, 2100]                                       # three stored chunks of 1000 per level
K_REQ = [1700, 900, 500]
B = 70                                                       # one full 64-replicate tile and a partial one


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


def _component_levels(M, seed=7, positive=False, n_samples=N):
    """_levels plus NaNs at other samples of the inner components: every component has a mask of its own"""
    levels = _levels(n_samples, M, seed=seed, positive=positive)
    for l, (f, c) in enumerate(levels):
        for m in range(1, M - 1):
            f[m, (3 + m)::(50 + 7 * m)] = np.nan
            if c is not None:
                c[m, (9 + 2 * m)::(120 + 11 * m)] = np.nan
    return levels


def _domains(M, lo=-2.0, hi=2.0):
    """a different domain per component: different samples fall outside"""
    return [(lo + 0.1 * (m % 7), hi + 0.15 * (m % 5)) for m in range(M)]


def _cases():
    from mlmc_amd import Legendre, Monomial, Fourier
    return {
        # name: (M, moments objects, positive data, replicates, components checked)
        "legendre": (5, lambda: [Legendre(7, d) for d in _domains(5)], False, B, range(5)),
        "monomial": (5, lambda: [Monomial(5, d) for d in _domains(5)], False, B, range(5)),
        "fourier": (5, lambda: [Fourier(6, d) for d in _domains(5)], False, B, range(5)),
        "legendre_log_mixed": (5, lambda: [Legendre(7, (0.2 + 0.02 * m, 6.0 + 0.3 * m), log=(m % 2 == 0)) for m in range(5)], True, B,
                               range(5)),
        "one_component": (1, lambda: [Legendre(7, (-2.0, 2.0))], False, B, range(1)),
        "forty_by_sixty": (40, lambda: [Legendre(60, d) for d in _domains(40, -2.5, 2.5)], False, 17, (0, 17, 39)),
    }


def _check_against_scalar(q, st, fns, k, seed, n_rep, res, comps, reps):
    """Component m of `res` against Estimate(scalar_component(q, m), st, fns[m]).est_bootstrap_batch: counts exactly, level means and
    variances within the bounds of the scalar route's own replicate test (1e-12 x sum w |d| / n and its variance form), the scales
    rebuilt from the explicit resample of the scalar component (the exported weights)."""
    from mlmc_amd.estimator import Estimate, scalar_component
    M = len(fns)
    for m in comps:
        qm = q if M == 1 else scalar_component(q, m)
        ref = Estimate(qm, st, fns[m]).est_bootstrap_batch(n_rep, sample_vector=k, seed=seed)
        assert np.array_equal(res.n_samples[:, :, m], ref.n_samples), m              # every replicate, exact integers
        for b in reps:
            lv = _resample_levels(qm, st, k, seed, n_rep, b)
            for l, (f, c) in enumerate(lv):
                vf = fns[m].eval_all(f)                                               # [1, n', R], NaN where masked
                vc = fns[m].eval_all(c) if c is not None else np.zeros_like(vf)
                keep = ~np.any(np.isnan(vf), axis=(0, 2)) & ~np.any(np.isnan(vc), axis=(0, 2))
                d = (vf - vc)[0, keep, :]
                n_l = int(keep.sum())
                assert res.n_samples[b, l, m] == n_l, (m, b, l)
                s1, s2 = np.sum(np.abs(d), axis=0), np.sum(d * d, axis=0)
                got_m, want_m = res.l_means[b, l, m], np.asarray(ref.l_means[b][l]).reshape(-1)
                got_v, want_v = res.l_vars[b, l, m], np.asarray(ref.l_vars[b][l]).reshape(-1)
                err = np.abs(got_m - want_m)
                print("m", m, "b", b, "l", l, "mean err / bound", float(np.max(err / (1e-12 * (s1 / max(n_l, 1)) + 1e-300))))
                assert np.all(err <= 1e-12 * (s1 / max(n_l, 1)) + 1e-300), (m, b, l, np.max(err))
                if n_l > 1:
                    tol_v = 1e-12 * (s2 + s1 * s1 / n_l) / (n_l - 1) + 1e-300
                    assert np.all(np.abs(got_v - want_v) <= tol_v), (m, b, l, np.max(np.abs(got_v - want_v) / tol_v))
                else:
                    assert np.all(np.isinf(got_v))
            # totals of the replicate: the same sums over the levels
            assert np.allclose(res.mean[b, m], np.asarray(ref.mean[b]).reshape(-1), rtol=1e-11, atol=1e-13)


# ---- 1. every component equals the scalar route ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(_cases()))
def test_components_equal_the_scalar_route(hip, case):
    from mlmc_amd.estimator import Estimate
    M, make_fns, positive, n_rep, comps = _cases()[case]
    fns = make_fns()
    R = fns[0].size
    st = _memory(_component_levels(M, positive=positive), M, chunk_size=1000)
    q = _root_q(st, M)
    res = Estimate(q, st, fns[0]).est_bootstrap_components(n_rep, sample_vector=K_REQ, moments_fns=fns, seed=2024)
    assert res.seed == 2024
    assert res.n_samples.shape == (n_rep, 3, M) and res.n_samples.dtype == np.int64
    assert res.l_means.shape == res.l_vars.shape == (n_rep, 3, M, R) and res.mean.shape == res.var.shape == (n_rep, M, R)
    if M > 1:
        assert len({tuple(res.n_samples[0, :, m]) for m in range(M)}) > 1              # the masks do differ
    _check_against_scalar(q, st, fns, K_REQ, 2024, n_rep, res, comps, sorted({0, n_rep // 2 - 2 if n_rep == B else 8, n_rep - 1}))


def test_default_moments_fn_serves_every_component(hip):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    st = _memory(_component_levels(3), 3, chunk_size=1000)
    q = _root_q(st, 3)
    fn = Legendre(4, (-2.0, 2.0))
    a = Estimate(q, st, fn).est_bootstrap_components(20, sample_vector=K_REQ, seed=5)
    b = Estimate(q, st).est_bootstrap_components(20, sample_vector=K_REQ, moments_fns=[fn] * 3, seed=5)
    for name in ("n_samples", "l_means", "l_vars", "mean", "var"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


# ---- 1b. the two routes of the library agree bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [9001, 40000])
@pytest.mark.parametrize("family", ["legendre", "monomial"])
def test_component_route_equals_one_component_route_bit_for_bit(hip, family, n):
    """mlmc_bootstrap_create_multi against mlmc_bootstrap_create on one row at a time, at the engine level: both routes evaluate the
    same term sequence, feed the same MFMA k-steps in the same order and add slices and ranges in the same fixed order, and a sample
    component m drops contributes exact zeros in both, so n, s and sp of component m are EQUAL whenever both cut the same sample
    ranges (M (K + 1) <= 256 and M <= 256).  M = 5, K = 7: 40 columns, JT = 4 and column blocks that straddle components against
    the 7 columns (JT = 1) of a single component; B = 70: a full and a partial 64-replicate tile; n = 9001: three tiles, partial
    last tile, 512-sample slice and 64-sample batch; n = 40000: two sample ranges in both routes.  A level-0 chunk and a pair."""
    import torch
    from mlmc_amd import Legendre, Monomial, engine
    from mlmc_amd.quantity import quantity_estimate as qe
    M, K, seed = 5, 7, 4711
    fns = [{"legendre": Legendre, "monomial": Monomial}[family](K, d) for d in _domains(M)]
    levels = [(torch.from_numpy(f).cuda(), None if c is None else torch.from_numpy(c).cuda())
              for f, c in _component_levels(M, seed=23, n_samples=[n, n])]
    rng = np.random.default_rng(n)
    sizes = [np.concatenate(([0, n, 1], rng.integers(0, n + 1, size=B - 3))) for _ in levels]

    def run(acc, rows):
        for l, (f, c) in enumerate(levels):
            acc.accum(l, f[rows].contiguous(), None if c is None else c[rows].contiguous(), sizes[l], seed, qe.bootstrap_stream(l, 0))
        out = acc.finalize()
        acc.close()
        return out
    n_all, s_all, sp_all = run(engine.ComponentBootstrapAccumulator(fns, K, 2, B), slice(0, M))
    assert np.all(n_all[0] == 0) and n_all[1].min() > 0                                # replicates 0 and 1 pick 0 and n samples
    assert len({tuple(n_all[1, :, m]) for m in range(M)}) > 1                          # the masks do differ
    for m in range(M):
        n_one, s_one, sp_one = run(engine.BootstrapAccumulator(fns[m], 1, 2, B), slice(m, m + 1))
        for name, got, want in (("n", n_all[:, :, m], n_one), ("s", s_all[:, :, m], s_one), ("sp", sp_all[:, :, m], sp_one)):
            diff = np.argwhere(got != want)
            print(family, n, "component", m, name, "differing elements", len(diff),
                  "first", None if not len(diff) else (tuple(diff[0]), got[tuple(diff[0])], want[tuple(diff[0])]))
            assert np.array_equal(got, want), (m, name)


# ---- 2. a planted mask ----------------------------------------------------------------------------------------------------------------
def test_planted_mask_counts_follow_the_weights(hip):
    from mlmc_amd import Legendre, engine
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    M, level, comp = 5, 1, 2
    fns = [Legendre(7, d) for d in _domains(M)]
    plain = _component_levels(M)
    planted = [(f.copy(), None if c is None else c.copy()) for f, c in plain]
    survivors = [17, 1203, 2399]                               # stored chunks 0, 1 and 2 of the level
    f, c = planted[level]
    inside = f[comp, survivors].copy(), c[comp, survivors].copy()
    f[comp, :] = 50.0                                          # outside the component's domain
    f[comp, survivors] = np.clip(np.nan_to_num(inside[0]), -1.0, 1.0)
    c[comp, survivors] = np.clip(np.nan_to_num(inside[1]), -1.0, 1.0)
    res = {}
    for name, levels in (("plain", plain), ("planted", planted)):
        st = _memory(levels, M, chunk_size=1000)
        res[name] = Estimate(_root_q(st, M), st, fns[0]).est_bootstrap_components(B, sample_vector=K_REQ, moments_fns=fns, seed=31)
    # the count of the planted component: the weights of its three surviving samples, exactly
    want = np.zeros(B, dtype=np.int64)
    for chunk in range(3):
        n_c = 1000 if chunk < 2 else N[level] - 2000
        sizes = qe.bootstrap_sizes(31, level, chunk, K_REQ[level], N[level], n_c, B)
        w = engine.bootstrap_weights(n_c, sizes, 31, qe.bootstrap_stream(level, chunk))
        want += w[:, survivors[chunk] - 1000 * chunk]
    assert np.array_equal(res["planted"].n_samples[:, level, comp], want)
    assert want.max() > 0
    # nobody else notices: the other components and the other levels of the planted one
    others = [m for m in range(M) if m != comp]
    assert np.array_equal(res["planted"].n_samples[:, :, others], res["plain"].n_samples[:, :, others])
    assert np.array_equal(res["planted"].l_means[:, :, others], res["plain"].l_means[:, :, others])
    assert np.array_equal(res["planted"].l_vars[:, :, others], res["plain"].l_vars[:, :, others], equal_nan=True)
    assert np.array_equal(res["planted"].n_samples[:, [0, 2], comp], res["plain"].n_samples[:, [0, 2], comp])


# ---- 3. determinism and the prefix property ----------------------------------------------------------------------------------------------
def test_bit_identical_runs_and_prefix(hip):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    M = 5
    fns = [Legendre(7, d) for d in _domains(M)]
    st = _memory(_component_levels(M), M, chunk_size=1000)
    est = Estimate(_root_q(st, M), st, fns[0])
    a = est.est_bootstrap_components(B, sample_vector=K_REQ, moments_fns=fns, seed=11)
    b = est.est_bootstrap_components(B, sample_vector=K_REQ, moments_fns=fns, seed=11)
    c = est.est_bootstrap_components(17, sample_vector=K_REQ, moments_fns=fns, seed=11)
    for name in ("n_samples", "l_means", "l_vars", "mean", "var"):
        x, y, z = getattr(a, name), getattr(b, name), getattr(c, name)
        assert np.array_equal(x, y, equal_nan=True), name
        assert np.array_equal(x[:17], z, equal_nan=True), name
    d = est.est_bootstrap_components(B, sample_vector=K_REQ, moments_fns=fns, seed=12)
    assert not np.array_equal(a.l_means, d.l_means)


def test_zero_requested_samples_at_a_level(hip):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate, scalar_component
    M = 3
    fns = [Legendre(4, d) for d in _domains(M)]
    st = _memory(_component_levels(M), M, chunk_size=1000)
    q = _root_q(st, M)
    r = Estimate(q, st, fns[0]).est_bootstrap_components(20, sample_vector=[600, 0, 300], moments_fns=fns, seed=1)
    ref = Estimate(scalar_component(q, 1), st, fns[1]).est_bootstrap_batch(20, sample_vector=[600, 0, 300], seed=1)
    assert np.all(r.n_samples[:, 1] == 0) and np.array_equal(r.n_samples[:, :, 1], ref.n_samples)
    assert np.all(np.isnan(r.l_means[:, 1])) and np.all(np.isinf(r.l_vars[:, 1])) and np.all(np.isnan(r.mean))
    assert np.all(np.isnan(ref.l_means[:, 1])) and np.all(np.isnan(ref.mean))


# ---- 4. storages and the device tree -----------------------------------------------------------------------------------------------------
def test_device_memory_storage(hip):
    import torch
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.sample_storage import DeviceMemory
    M = 3
    levels = _component_levels(M, seed=31)
    dev = DeviceMemory()
    dev.save_global_data(result_format=_spec(M), level_parameters=[[0.5], [0.1], [0.02]])
    for l, (f, c) in enumerate(levels):
        pairs = np.stack([f, np.zeros_like(f) if c is None else c], axis=-1)
        dev.set_level_samples(l, torch.from_numpy(pairs).cuda())
    qe.device_cache_clear()
    fns = [Legendre(6, d) for d in _domains(M)]
    q = _root_q(dev, M)
    k = [1000, 500, 400]
    res = Estimate(q, dev, fns[0]).est_bootstrap_components(B, sample_vector=k, moments_fns=fns, seed=8)
    _check_against_scalar(q, dev, fns, k, 8, B, res, range(M), (0, 69))
    qe.device_cache_clear()


def test_derived_vector_quantity_on_the_device_tree(hip):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    M = 3
    st = _memory(_component_levels(M, seed=41), M, chunk_size=1000)
    fns = [Legendre(6, (-3.0 + 0.2 * m, 5.0 + 0.3 * m)) for m in range(M)]
    os.environ["MLMC_HIP_DEVICE_TREE"] = "1"
    try:
        qe.device_cache_clear()
        q = _root_q(st, M) * 2 + 1
        res = Estimate(q, st, fns[0]).est_bootstrap_components(B, sample_vector=K_REQ, moments_fns=fns, seed=6)
        _check_against_scalar(q, st, fns, K_REQ, 6, B, res, range(M), (0, 69))
    finally:
        os.environ.pop("MLMC_HIP_DEVICE_TREE", None)
        qe.device_cache_clear()


# ---- 5. quantile bands ----------------------------------------------------------------------------------------------------------------------
PROBS = np.array([0.05, 0.5, 0.95])


def _band_case():
    """M = 4 near-normal components with their own centres and widths, no NaNs; Legendre R = 9 on the domains estimate_domains gives"""
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    M = 4
    rng = np.random.default_rng(19)
    levels = []
    for l, n in enumerate(N):
        f = (1.0 + 0.25 * np.arange(M))[:, None] * rng.normal(size=(M, n)) + 0.3 * np.arange(M)[:, None]
        c = None if l == 0 else f + 0.05 * 0.5 ** l * rng.normal(size=(M, n))
        levels.append((f, c))
    st = _memory(levels, M, chunk_size=1000)
    q = _root_q(st, M)
    fns = [Legendre(9, tuple(d)) for d in Estimate.estimate_domains(q, st)]
    return st, q, fns


def test_quantile_bands_step_by_step(hip):
    from mlmc_amd.estimator import Estimate, quantile_bands
    from mlmc_amd.tool import simple_distribution as sd
    st, q, fns = _band_case()
    M, R = len(fns), 9
    est = Estimate(q, st, fns[0])
    dens = est.construct_densities(moments_fns=fns)
    bands = est.bootstrap_component_quantiles(PROBS, n_subsamples=B, sample_vector=K_REQ, seed=77, level=0.9, moments_fns=fns,
                                              densities=dens)
    assert bands.seed == 77 and bands.replicates.shape == (B, M, 3) and bands.success.shape == (B, M)
    assert bands.success.dtype == bool and np.array_equal(bands.n_ok, bands.success.sum(axis=0))
    # q: the quantiles of the full sample
    assert np.array_equal(bands.q, est.estimate_component_quantiles(PROBS, densities=dens)[0])
    # replicates: the single solve of the moments rebuilt from the replicate's level sums, bit for bit
    reps = est.est_bootstrap_components(B, sample_vector=K_REQ, moments_fns=fns, seed=77)
    for b in (0, 33, 69):
        for m in range(M):
            mobj = dens[m][3]
            # s / n is the level mean of engine.level_stats: the formula of step 3 from the public result
            mu = np.sum([reps.l_means[b, l, m, :R] @ mobj._base_matrix.T for l in range(3)], axis=0)
            d = sd.SimpleDistribution(mobj, np.stack((mu, np.ones(mobj.size)), axis=1), domain=mobj.domain)
            result = sd.estimate_densities_minimize([d], 1e-8, 0.0)[0]
            single = np.asarray(sd.quantiles([d], PROBS)[0])
            print("b", b, "m", m, "single solve success", bool(result.success), "quantiles", single, bands.replicates[b, m])
            assert bool(result.success), (b, m)
            assert bands.success[b, m], (b, m)
            assert np.array_equal(bands.replicates[b, m], single), (b, m)
    # bands: the host helper over the replicates; the full-sample quantile lies inside the replicates' range (seeded call)
    lo, hi = quantile_bands(bands.replicates, bands.success, 0.9)
    assert np.array_equal(bands.lo, lo) and np.array_equal(bands.hi, hi)
    assert np.all(bands.lo <= bands.hi)
    for m in range(M):
        ok = bands.replicates[bands.success[:, m], m]
        assert ok.shape[0] > 0
        assert np.all(ok.min(axis=0) <= bands.q[m]) and np.all(bands.q[m] <= ok.max(axis=0)), m
    # computed densities and default moments_fns: the same call
    again = est.bootstrap_component_quantiles(PROBS, n_subsamples=B, sample_vector=K_REQ, seed=77, densities=dens)
    assert np.array_equal(again.replicates, bands.replicates) and np.array_equal(again.success, bands.success)


# ---- 6. errors of the device route ---------------------------------------------------------------------------------------------------------
def test_a_fully_masked_component_raises(hip):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    M = 3
    st = _memory(_component_levels(M), M, chunk_size=1000)
    fns = [Legendre(4, (-2.0, 2.0)), Legendre(4, (100.0, 101.0)), Legendre(4, (-2.0, 2.0))]
    with pytest.raises(Exception, match="All samples were masked"):
        Estimate(_root_q(st, M), st, fns[0]).est_bootstrap_components(5, moments_fns=fns, seed=2)


def test_totals_over_two_gib_are_refused_at_create(hip):
    from mlmc_amd import Legendre, engine
    fns = [Legendre(64, (-2.0, 2.0))] * 64
    with pytest.raises(hip.MlmcHipError, match=r"mlmc_bootstrap_create_multi: the totals .* at most 2048 MiB"):
        engine.ComponentBootstrapAccumulator(fns, 64, 5, 10_000)          # 5 x 10^4 x 64 x 129 doubles = 3.1 GiB
    engine.ComponentBootstrapAccumulator(fns, 64, 5, 300).close()         # 95 MiB


def test_create_multi_argument_errors(hip):
    from mlmc_amd import Legendre, Monomial, engine
    from mlmc_amd.moments import Spline
    leg = Legendre(6, (-2.0, 2.0))
    for fns, K, match in (([leg, Monomial(6, (-2.0, 2.0))], 6, "component 1: every component must use the same family"),
                          ([leg, Legendre(4, (-2.0, 2.0))], 6, "component 1: basis smaller than K"),
                          ([Spline(6, (-2.0, 2.0))], 6, "component 0: only Legendre, monomial and Fourier moments"),
                          ([leg], 0, "K must be in 1..512")):
        with pytest.raises(hip.MlmcHipError, match="mlmc_bootstrap_create_multi: " + match):
            engine.ComponentBootstrapAccumulator(fns, K, 2, 5)


def test_finalize_refuses_the_other_kind_of_handle(hip):
    from mlmc_amd import Legendre, engine
    fn = Legendre(4, (-2.0, 2.0))
    lib = hip.lib()
    n = np.zeros((3, 2, 2), dtype=np.int64)
    s = np.zeros((3, 2, 2, 4))
    sp = np.zeros_like(s)
    multi = engine.ComponentBootstrapAccumulator([fn, fn], 4, 2, 3)
    single = engine.BootstrapAccumulator(fn, 2, 2, 3)
    try:
        with pytest.raises(hip.MlmcHipError, match="mlmc_bootstrap_finalize: the handle comes from mlmc_bootstrap_create_multi"):
            hip.check(lib.mlmc_bootstrap_finalize(multi._h, hip.ptr(n), hip.ptr(s), hip.ptr(sp)))
        with pytest.raises(hip.MlmcHipError, match="mlmc_bootstrap_finalize_multi: the handle comes from mlmc_bootstrap_create "):
            hip.check(lib.mlmc_bootstrap_finalize_multi(single._h, hip.ptr(n), hip.ptr(s), hip.ptr(sp)))
        # both still serve their own finalize (nothing accumulated: zeros)
        out = multi.finalize()
        assert out[0].shape == (3, 2, 2) and not out[0].any() and not out[1].any()
        assert not single.finalize()[0].any()
    finally:
        multi.close()
        single.close()
