"""CPU tests of the host-side logic of the drop-in API: quantity tree bookkeeping, Memory storage, sample allocation,
variance regression, orthogonalisation -- everything that needs no kernel."""
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _spec():
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    return [QuantitySpec(name="length", unit="m", shape=(2, 1), times=[1, 2, 3], locations=['10', '20']),
            QuantitySpec(name="width", unit="mm", shape=(2, 1), times=[1, 2, 3], locations=['30', '40'])]


def _storage(n=(7, 5, 3)):
    from mlmc_amd.sample_storage import Memory
    st = Memory()
    st.save_global_data(result_format=_spec(), level_parameters=[[0.1], [0.01], [0.001]])
    rng = np.random.default_rng(0)
    M = 24
    for l, nl in enumerate(n):
        samples = [("L{:02d}_S{:07d}".format(l, i), (rng.normal(size=M), rng.normal(size=M) if l else np.zeros(M))) for i in range(nl)]
        st.save_samples({l: samples}, {l: []})
    st.save_n_ops([(0, (10.0, 7)), (1, (50.0, 5)), (2, (90.0, 3))])
    return st


def test_memory_storage_and_quantity_selection():
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.quantity.quantity_spec import ChunkSpec
    st = _storage()
    assert st.get_n_levels() == 3 and st.get_n_collected() == [7, 5, 3] and st.get_level_ids() == [0, 1, 2]
    assert np.allclose(st.get_n_ops(), [10 / 7, 10.0, 30.0])
    chunks = list(st.chunks())
    assert [c.level_id for c in chunks] == [0, 1, 2] and chunks[1].chunk_slice == slice(0, 5, 1)
    assert st.sample_pairs_level(ChunkSpec(level_id=0)).shape == (24, 7, 1)
    assert st.sample_pairs_level(chunks[1]).shape == (24, 5, 2)
    root = make_root_quantity(st, _spec())
    assert root.size() == 24
    length = root['length']
    assert length.size() == 12
    loc = length[2]['20']
    assert loc.size() == 2
    raw = st.sample_pairs_level(chunks[2])
    # 'length' starts at 0; time 2 is the second block of 4; location '20' the second pair; flat index 4 + 2 = 6..7
    assert np.array_equal(loc.samples(chunks[2]), raw[6:8])
    assert np.array_equal(loc[1].samples(chunks[2]), raw[7:8])
    width = root['width'][3]['30'][0]
    assert np.array_equal(width.samples(chunks[1]), st.sample_pairs_level(chunks[1])[12 + 8:12 + 9])
    # arithmetic, constants, ufuncs, masks
    q = 2 * loc[0] + 1.0
    assert np.allclose(q.samples(chunks[1]), 2 * raw_l1(st, 6) + 1.0)
    assert np.allclose(np.sin(loc[0]).samples(chunks[1]), np.sin(raw_l1(st, 6)))
    mask = loc[0] > 0.0
    sel = loc.select(mask)
    got = sel.samples(chunks[1])
    r = st.sample_pairs_level(chunks[1])[6:8]
    keep = (r[0] > 0).all(axis=-1)
    assert got.shape == (2, int(keep.sum()), 2) and np.array_equal(got, r[:, keep, :])
    with pytest.raises(Exception):
        loc.select(loc[0])          # not a BoolType quantity
    interp = length.time_interpolation(1.5)
    assert interp.size() == 4
    assert np.allclose(interp.samples(chunks[1]), 0.5 * (st.sample_pairs_level(chunks[1])[0:4] + st.sample_pairs_level(chunks[1])[4:8]))


def raw_l1(st, idx):
    return st.sample_pairs_level(list(st.chunks())[1])[idx:idx + 1]


def test_quantity_mean_container():
    from mlmc_amd.quantity import quantity_types as qt
    from mlmc_amd.quantity.quantity import QuantityMean
    qtype = qt.ArrayType((2, 3), qt.ScalarType())
    l_means = np.arange(12, dtype=float).reshape(2, 6)
    l_vars = np.ones((2, 6))
    qm = QuantityMean(qtype, l_means, l_vars, n_samples=[10, 5], n_rm_samples=[1, 0])
    assert qm.mean.shape == (2, 3) and np.array_equal(qm.mean.ravel(), l_means.sum(axis=0))
    assert np.allclose(qm.var, 0.1 + 0.2)
    assert qm.l_means.shape == (2, 2, 3)
    sub = qm[1]
    assert sub.mean.shape == (3,) and np.array_equal(sub.mean, qm.mean[1])


def test_allocation_and_regression_host_functions():
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate, estimate_n_samples_for_target_variance, determine_level_parameters, \
        determine_n_samples, determine_sample_vec, calc_level_params
    with open(os.path.join(GOLDEN, "G4_alloc.json")) as f:
        g4 = json.load(f)
    est = Estimate(None, None, Legendre(5, (-1.0, 1.0)))
    for key, d in g4.items():
        if not isinstance(d, dict):
            continue
        raw = np.array(d["raw_vars"])
        reg = est._all_moments_variance_regression(raw, np.array(d["steps"]))
        assert np.allclose(reg, np.array(d["reg_vars"]), rtol=1e-12, atol=0)
        n_est = estimate_n_samples_for_target_variance(1e-6, np.array(d["reg_vars"]), d["n_ops"], len(raw))
        assert np.array_equal(n_est, d["n_estimated"])
        n_est = estimate_n_samples_for_target_variance(1e-5, raw, d["n_ops"], len(raw))
        assert np.array_equal(n_est, d["n_estimated_raw"])
    assert determine_level_parameters(5, [0.5, 0.01]) == g4["level_params_5"]
    assert calc_level_params([0.5, 0.01], 1) == g4["level_params_1"]
    assert determine_n_samples(5).tolist() == g4["determine_n_samples_5"]
    assert determine_n_samples(4, [1000, 10]).tolist() == g4["determine_n_samples_4_1000_10"]
    assert determine_sample_vec([5, 4, 3], 2).tolist() == [5, 4]
    # closed form of Var[log(chi2_df/df)] used in place of the reference's adaptive quadratures (estimator.py:136-169)
    import scipy.integrate as integrate
    import scipy.stats as st
    est._n_created_samples = [30, 8]
    got = est._variance_of_variance()
    for ns, v in zip([30, 8], got):
        df = ns - 1
        pdf = lambda x: np.exp(x) * df * st.chi2.pdf(np.exp(x) * df, df=df)
        m1 = integrate.quad(lambda x: x * pdf(x), -30, 10)[0]
        m2 = integrate.quad(lambda x: x * x * pdf(x), -30, 10)[0]
        assert abs(v - (m2 - m1 ** 2)) < 1e-7


def test_orthogonal_moments_host():
    from mlmc_amd import Legendre, TransformedMoments
    from mlmc_amd.tool import simple_distribution as sd
    g5 = np.load(os.path.join(GOLDEN, "G5_ortho.npz"))
    for name in ("norm12", "norm110", "lognorm"):
        for R in (7, 21, 41):
            key = f"{name}_R{R}"
            base = Legendre(R, tuple(g5[key + "_domain"]))
            cov = g5[key + "_cov"]
            for tol in (1e-4, 0.0):
                ortho, (ev, thr, L) = sd.construct_ortogonal_moments(base, cov, tol)
                tk = key + "_tol{:g}".format(tol)
                assert isinstance(ortho, TransformedMoments) and ortho.size == L.shape[0]
                assert thr == int(g5[tk + "_threshold"])
                assert np.allclose(L, g5[tk + "_L"], rtol=1e-7, atol=1e-9)
            ortho, (ev, thr, L) = sd.construct_ortogonal_moments(base, cov, 1e-4)
            assert np.linalg.norm(L @ cov @ L.T - np.eye(L.shape[0])) < 1e-8      # test/test_distribution.py:180 (1e-10 there on exact cov)
            # tol=None: the slope-change threshold (simple_distribution.py:781-782) on exact and perturbed covariances
            for tag in ("none", "none_n6", "none_n4"):
                tk = key + "_tol" + tag
                ortho2, (ev2, thr2, L2) = sd.construct_ortogonal_moments(base, g5[tk + "_cov"].copy(), tol=None)
                assert thr2 == int(g5[tk + "_threshold"]), tk
                assert np.allclose(ev2, g5[tk + "_eval"], rtol=1e-9, atol=1e-13)
                assert L2.shape == g5[tk + "_L"].shape and np.allclose(L2, g5[tk + "_L"], rtol=1e-6, atol=1e-8), tk
                assert ortho2.size == L2.shape[0]


def test_moments_objects_host_side():
    from mlmc_amd import Legendre, Monomial, Fourier, TransformedMoments
    fn = Legendre(5, (1.0, 3.0))
    assert fn.size == 5 and fn.domain == (1.0, 3.0) and fn.ref_domain == (-1, 1)
    assert fn._linear_scale == 1.0 and fn._linear_shift == 1.0
    assert fn == Legendre(5, (1.0, 3.0)) and not (fn == Legendre(6, (1.0, 3.0))) and not (fn == Monomial(5, (1.0, 3.0)))
    assert fn.change_size(9).size == 9 and isinstance(fn.change_size(9), Legendre)
    assert np.allclose(fn.inv_transform(np.array([-1.0, 0.0, 1.0])), [1.0, 2.0, 3.0])
    assert fn.diff_mat.shape == (5, 5) and fn.diff_mat[0, 1] == 1 and fn.diff_mat[1, 2] == 3 and fn.diff_mat[0, 3] == 1
    lg = Monomial(3, (1.0, np.e), log=True)
    assert np.isclose(lg._linear_shift, 0.0) and np.isclose(lg._linear_scale, 1.0)
    assert Fourier(6).ref_domain == (0, 2 * np.pi)
    with pytest.raises(AssertionError):
        Legendre(0, (0, 1))
    with pytest.raises(AssertionError):
        Legendre(3, (1.0, 1.0))
    tm = TransformedMoments(fn, np.eye(3, 5))
    assert tm.size == 3 and tm.domain == fn.domain
    tm2 = TransformedMoments(tm, np.ones((2, 3)))
    assert tm2._base is fn and np.array_equal(tm2._base_matrix, np.ones((2, 3)) @ np.eye(3, 5))
    with pytest.raises(AssertionError):
        TransformedMoments(fn, np.eye(3, 4))


def test_synth_device_storage_interface_without_gpu():
    """Bookkeeping of SynthDeviceStorage (chunks, shards, costs, result format) needs no device."""
    from mlmc_amd.sim.synth_device import SynthDeviceStorage, n_ops_estimate, result_format
    st = SynthDeviceStorage([[0.5], [0.1], [0.02]], [1000, 500, 250], chunk_size=400)
    assert st.get_n_levels() == 3 and st.get_level_ids() == [0, 1, 2] and st.get_n_collected() == [1000, 500, 250]
    assert st.get_level_parameters() == [[0.5], [0.1], [0.02]]
    chunks = list(st.chunks())
    assert [(c.level_id, c.chunk_slice.start, c.chunk_slice.stop) for c in chunks] == \
        [(0, 0, 400), (0, 400, 800), (0, 800, 1000), (1, 0, 400), (1, 400, 500), (2, 0, 250)]
    assert [c.chunk_slice.stop for c in st.chunks(level_id=0, n_samples=450)] == [400, 450]
    assert np.allclose(st.get_n_ops(), [n_ops_estimate(h) for h in (0.5, 0.1, 0.02)])
    assert np.isclose(n_ops_estimate(0.1), 100 * np.log(10.0))                    # synth_simulation.py:133-134
    fmt = result_format()
    assert [q.name for q in fmt] == ["length", "width"] and fmt[0].shape == (2, 1) and fmt[0].times == [1, 2, 3]
    # shards: contiguous slices of every level (engine.shard_bounds), together the whole level
    parts = [SynthDeviceStorage([[0.5], [0.1]], [1001, 77], shard=(r, 4)) for r in range(4)]
    assert [sum(p.get_n_collected()[l] for p in parts) for l in range(2)] == [1001, 77]
    assert [p._first[0] for p in parts] == [0, 250, 500, 750]
    with pytest.raises(NotImplementedError):
        st.save_samples({}, {})


def test_device_sampler_follows_the_reference_scheduling():
    """DeviceSampler bookkeeping (no GPU: samples are generated only when read) replays the reference's adaptive loop
    (Sampler + OneProcessPool, tests/golden/G9_sampler_loop.json from oracle/gen_golden.py g9): fed the recorded
    n_estimated of every round it reproduces scheduled counts, the counts that reached the storage, and the flag."""
    import json
    import os
    from mlmc_amd.sampler import DeviceSampler
    from mlmc_amd.sim.synth_device import SynthDeviceStorage
    with open(os.path.join(os.path.dirname(__file__), "golden", "G9_sampler_loop.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) == 3
    for case in cases:
        steps = case["level_parameters"]
        st = SynthDeviceStorage(steps, [0] * len(steps), loc=case["loc"], scale=case["scale"])
        sampler = DeviceSampler(st, level_parameters=steps)
        sampler.set_initial_n_samples(case["initial"])
        sampler.schedule_samples()
        assert sampler.ask_sampling_pool_for_samples() == 0
        assert [int(v) for v in sampler.l_scheduled_samples()] == case["initial_scheduled"]
        assert st.get_n_collected() == case["initial_scheduled"]
        for rnd in case["rounds"]:
            done = sampler.process_adding_samples(np.array(rnd["n_estimated"]), 0, 0.1)
            assert [int(v) for v in sampler.l_scheduled_samples()] == rnd["n_scheduled"], case["name"]
            assert [int(v) for v in sampler.n_finished_samples] == rnd["n_finished"], case["name"]
            assert done == rnd["done"]
        assert st.get_n_collected() == case["n_collected"]
    # a level never shrinks; timeout <= 0 means "do not wait"
    sampler.set_level_target_n_samples([1] * sampler.n_levels)
    sampler.schedule_samples()
    assert [int(v) for v in sampler.l_scheduled_samples()] == cases[-1]["rounds"][-1]["n_scheduled"]
    assert sampler.ask_sampling_pool_for_samples(timeout=0) == 1
    assert sampler.sample_range(1000, 10).tolist() == [1000, 316, 100, 32, 10]


def test_block_upload_layout_decisions():
    """quantity_estimate._block_layout: which host views of a storage chunk go up as one flat copy (strided LOAD on the
    device) and with which strides; pure shape / stride arithmetic, checked by rebuilding the view from the flat span."""
    from mlmc_amd.quantity.quantity_estimate import _block_layout
    rng = np.random.default_rng(3)

    def check(raw, n_rows_read, expect_block):
        got = _block_layout(raw, n_rows_read)
        assert (got is not None) == expect_block, (raw.shape, raw.strides, got)
        if got is None:
            return
        span, sn, sw = got
        flat = np.lib.stride_tricks.as_strided(raw, shape=(span,), strides=(8,))
        m_total, n, width = raw.shape
        for m in (0, m_total - 1):
            for i in (0, n // 2, n - 1):
                for side in range(width):
                    assert flat[m + i * sn + side * sw] == raw[m, i, side]

    store = rng.normal(size=(1000, 2, 24))                        # Memory / HDF5 layout [N, 2, M]
    chunk = store[100:600]
    check(chunk.transpose(2, 0, 1), 24, True)                     # a pair level, every row read
    check(chunk.transpose(2, 0, 1), 3, True)                      # 3 of 24 rows: 3 * 8 >= 24
    check(chunk.transpose(2, 0, 1), 2, False)                     # 2 of 24 rows: per-row uploads
    check(chunk[:, :1, :].transpose(2, 0, 1), 24, True)           # level 0 view [n, 1, M] of the same records
    one = rng.normal(size=(500, 2, 1))
    check(one.transpose(2, 0, 1), 1, False)                       # M = 1 pairs: raw[0] already is an [n][2] row
    check(one[:, :1, :].transpose(2, 0, 1), 1, True)              # M = 1 at level 0: fine values at stride 2
    check(np.ascontiguousarray(chunk.transpose(2, 0, 1)), 24, False)      # a copy in [M][n][2] order: not a record array
    check(chunk.transpose(2, 0, 1)[:, ::-1], 24, False)           # reversed samples
    check(chunk.transpose(2, 0, 1)[:, ::7], 24, False)            # every 7th sample: the span would be 7x the data
    check(chunk.transpose(2, 0, 1)[:, ::2], 24, True)             # every 2nd: still within 3x
    check(chunk.transpose(2, 0, 1)[:, :0], 24, False)             # no samples
    check(chunk.astype(np.float32).transpose(2, 0, 1), 24, False)


def test_device_chunk_cache_accounting(monkeypatch):
    """The LRU bookkeeping of the HBM chunk cache (no GPU: entries are stand-ins that only report their size)."""
    from mlmc_amd.quantity.quantity_estimate import _DeviceChunkCache

    class Fake:
        def __init__(self, n):
            self.n = n

        def numel(self):
            return self.n

    monkeypatch.setenv("MLMC_HIP_DEVICE_CACHE_GB", str(1000 * 8 / 2 ** 30))     # room for 1000 doubles
    cache = _DeviceChunkCache()
    a, b = object(), object()
    cache.put_tensors("k1", Fake(300), Fake(100), owner=a)
    cache.put_tensors("k2", Fake(300), None, owner=b)
    cache.put_tensors("k3", Fake(200), None, owner=a)
    assert cache._bytes == 900 * 8 and list(cache._items) == ["k1", "k2", "k3"]
    assert cache.get("k1") is not None and list(cache._items) == ["k2", "k3", "k1"]      # a hit renews the entry
    cache.put_tensors("k4", Fake(350), None, owner=b)                                    # evicts the oldest entry, k2
    assert list(cache._items) == ["k3", "k1", "k4"] and cache._bytes == 950 * 8
    cache.put_tensors("k4", Fake(100), None, owner=b)                                    # replacing returns the old bytes
    assert cache._bytes == 700 * 8
    big = cache.put_tensors("k5", Fake(5000), None, owner=a)                             # over the budget: served, not kept
    assert big[2] == 5000 * 8 and "k5" not in cache._items and cache._bytes == 700 * 8
    cache.drop_owner(a)
    assert list(cache._items) == ["k4"] and cache._bytes == 100 * 8
    cache.clear()
    assert cache._bytes == 0 and not cache._items and cache.get("k4") is None


def test_level_stats_beyond_two_to_the_53_equal_the_reference_formula():
    """n = 1e8 samples per level (BASELINE configs[3]): s = sum of P_0 differences = n at level 0, and s * s = 1e16 passes
    2^53, so var_0 = (sp - s^2 / n) / (n - 1) is no longer exactly 0 for every n -- in the reference's own formula
    (quantity_estimate.py:72-77) just as here.  engine.level_stats must equal the oracle's restatement of that formula bit
    for bit, whatever it gives; `vars[0] == 0` exactly is guaranteed only while n^2 < 2^53, i.e. n < 9.49e7 per level."""
    from mlmc_amd.engine import level_stats
    from oracle import oracle_np as onp
    rng = np.random.default_rng(3)
    for n0 in (94_906_265, 94_906_267, 100_000_000, 99_987_653, 500_000_000):
        n = np.array([n0, n0 - 12345, 7])
        s = np.stack([n.astype(np.float64), rng.normal(size=3) * np.sqrt(n)], axis=1)       # column 0: phi_0 = 1 at level 0 ...
        s[1:, 0] = 0.0                                                                       # ... and differences 0 above
        sp = np.stack([n.astype(np.float64), np.abs(rng.normal(size=3)) * n], axis=1)
        sp[1:, 0] = 0.0
        l_means, l_vars = level_stats(n, s, sp)
        ref_means, ref_vars = onp.level_stats(s, sp, n)
        assert np.array_equal(l_means, ref_means) and np.array_equal(l_vars, ref_vars)
        assert l_means[0, 0] == 1.0
        if n0 <= 94_906_265:                      # floor(sqrt(2^53)): n * n is still exact
            assert l_vars[0, 0] == 0.0


def test_reference_estimate_density_root_variant_cannot_run_as_written():
    """Why mlmc_amd.tool.distribution.Distribution.estimate_density has no golden vector: the reference's method
    (distribution.py:159-181) calls `self._initialize_params(tol)`, whose signature is `(self, size, tol=None)` and which
    asserts `tol is not None` (:216-223).  The reference's own run of the method is recorded in G11 (oracle/gen_golden.py):
    it stops with that assertion in `_initialize_params`, with `size` bound to the tolerance and `tol` left None."""
    with open(os.path.join(GOLDEN, "G11_estimate_density_root.json")) as f:
        g11 = json.load(f)
    assert g11["raised"] == "AssertionError"
    assert g11["frames"] == ["estimate_density", "_initialize_params"]
    assert g11["raising_frame_args"] == {"size": g11["tol"], "tol": None}


def test_orthogonal_moments_of_128_moments_with_the_mrrr_driver(monkeypatch):
    """construct_ortogonal_moments switches to LAPACK's dsyevr for matrices of 96 rows and more (2.5 x faster at 128): same
    thresholds, same L to rounding as with NumPy's eigh (the reference's call, simple_distribution.py:768), and the
    reference's own quality bound ||L cov L^T - I|| < 1e-10 on the kept block (test/test_distribution.py:180)."""
    import scipy.linalg
    from mlmc_amd import Legendre
    from mlmc_amd.tool import simple_distribution as sd
    R = 128
    x, w = np.polynomial.legendre.leggauss(400)
    dens = np.exp(-0.5 * (3.7 * x) ** 2)
    dens /= np.sum(w * dens)
    P = np.polynomial.legendre.legvander(x, R - 1)
    cov = (P * (w * dens)[:, None]).T @ P                      # exact moment covariance of a truncated normal on (-3.7, 3.7)
    fn = Legendre(R, (-3.7, 3.7))
    got, (ev1, thr1, L1) = sd.construct_ortogonal_moments(fn, cov, tol=1e-10)
    monkeypatch.setattr(scipy.linalg, "eigh", lambda a, driver=None: np.linalg.eigh(a))
    _, (ev2, thr2, L2) = sd.construct_ortogonal_moments(fn, cov, tol=1e-10)
    assert thr1 == thr2 and got.size == R - thr1
    assert np.allclose(ev1, ev2, rtol=0, atol=1e-13)
    # a row of L (one orthogonal moment) is fixed up to its sign: the RQ factor inherits the signs LAPACK gives the
    # eigenvectors, which no driver normalises (the reference fixes only the sign of L[0, 0], simple_distribution.py:838-841)
    flip = np.sign(np.sum(L1 * L2, axis=1))
    assert np.all(flip != 0) and flip[0] == 1.0
    assert np.max(np.abs(L1 - flip[:, None] * L2)) <= 1e-6 * np.max(np.abs(L2))
    assert np.linalg.norm(L1 @ cov @ L1.T - np.eye(L1.shape[0])) < 1e-8
