"""GPU tests of the per-component moment estimates of a vector quantity: mlmc_accum_estimate_multi_var level sums against the
scalar estimates and the NumPy oracle, Estimate.estimate_component_moments / _diff_vars / _diff_vars_regression against the loop
of scalar estimates, a chunk of several sample blocks, the adaptive sample-allocation loop end to end, ABI errors; the mean-only entry (mlmc_accum_estimate_multi) against the variance
entry bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_density_batch import LOG_COMP, _components, _vector_levels, _vector_storage

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


def _fns(kind, R, doms):
    from mlmc_amd import Legendre, Monomial, Fourier
    cls = {"legendre": Legendre, "monomial": Monomial, "fourier": Fourier}[kind]
    return [cls(R, dom, log=(m == LOG_COMP)) for m, dom in enumerate(doms)]


CASES = [("legendre", R) for R in (1, 7, 25, 32, 33, 64, 100)] + [("monomial", 9), ("fourier", 11)]


@pytest.mark.parametrize("chunk_size", [None, 1500])
def test_level_sums_against_the_scalar_estimates_and_the_oracle(hip, chunk_size):
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    from oracle import oracle_np as onp
    levels, _ = _vector_levels()
    st, spec = _vector_storage(chunk_size)
    root, comps = _components(st, spec)
    doms = [Estimate.estimate_domain(q_m, st) for q_m in comps]
    kinds = {"legendre": onp.LEGENDRE, "monomial": onp.MONOMIAL, "fourier": onp.FOURIER}
    for kind, R in CASES:
        fns = _fns(kind, R, doms)
        n, n_rm, s, sp = qe.component_level_sums(root, fns)
        assert n.shape == n_rm.shape == (3, 6) and s.shape == sp.shape == (3, 6, R)
        for m, (q_m, fn) in enumerate(zip(comps, fns)):
            ref = qe.estimate_mean(qe.moments(q_m, fn))
            assert np.array_equal(n[:, m], ref.n_samples) and np.array_equal(n_rm[:, m], ref.n_rm_samples), (kind, R, m)
            if kind == "fourier":                  # the oracle's Fourier rows take 1-D input only: the scalar chain's sums
                oref = _scalar_chain(fn, [(f[m], None if c is None else c[m]) for f, c in levels])
            else:
                b = onp.Basis(kinds[kind], R, fn.domain, log=(m == LOG_COMP))
                chunks = []
                for l, (f, c) in enumerate(levels):
                    x = f[m][:, None] if c is None else np.stack([f[m], c[m]], axis=-1)
                    chunks.append([x[None]])
                oref = onp.estimate_mean(chunks, lambda x: onp.moments_rows(b, x))
            assert np.array_equal(n[:, m], oref.n_samples) and np.array_equal(n_rm[:, m], oref.n_rm_samples), (kind, R, m)
            scale = np.sqrt(np.abs(oref.sums_sq) * oref.n_samples[:, None]) + 1e-300
            assert np.all(np.abs(s[:, m, :] - oref.sums) <= 1e-10 * np.maximum(np.abs(oref.sums), scale)), (kind, R, m)
            assert np.all(np.abs(sp[:, m, :] - oref.sums_sq) <= 1e-10 * np.maximum(np.abs(oref.sums_sq), 1e-300) + 1e-13), \
                (kind, R, m)
    # the keep rule differs per component: the NaNs of component 1 do not drop samples of component 0
    assert n[0, 0] > n[0, 1]


def _scalar_chain(fn, levels):
    """n / n_rm / sums / sums_sq of the scalar accumulator (mlmc_accum_push) over one component's [n] level arrays."""
    import types
    from mlmc_amd.engine import LevelAccumulator
    acc = LevelAccumulator(fn, len(levels))
    for l, (f, c) in enumerate(levels):
        acc.push(l, np.ascontiguousarray(f), None if c is None else np.ascontiguousarray(c))
    n, n_rm, s, sp = acc.finalize()
    return types.SimpleNamespace(n_samples=n, n_rm_samples=n_rm, sums=s, sums_sq=sp)


def _loop(comps, st, fns, n_created):
    from mlmc_amd.estimator import Estimate
    out = []
    for q_m, fn in zip(comps, fns):
        e = Estimate(q_m, st, fn)
        mean, var = e.estimate_moments()
        l_vars, n_s = e.estimate_diff_vars()
        reg, n_ops = Estimate(q_m, st, fn).estimate_diff_vars_regression(n_created)
        out.append((np.asarray(mean), np.asarray(var), np.asarray(l_vars), np.asarray(n_s), reg, n_ops))
    return out


@pytest.mark.parametrize("chunk_size", [None, 1500])
def test_api_against_the_loop_of_scalar_estimates(hip, chunk_size):
    from mlmc_amd import Legendre, Spline
    from mlmc_amd.estimator import Estimate
    st, spec = _vector_storage(chunk_size)
    root, comps = _components(st, spec)
    doms = [Estimate.estimate_domain(q_m, st) for q_m in comps]
    n_created = [20000, 4000, 1200]
    for fns in (_fns("legendre", 13, doms), _fns("monomial", 6, doms), _fns("fourier", 9, doms),
                [Spline(10, dom) for dom in doms]):
        est = Estimate(root, st, fns[0])
        means, vars_ = est.estimate_component_moments(moments_fns=fns)
        l_vars, n_s = est.estimate_component_diff_vars(moments_fns=fns)
        reg, n_ops = est.estimate_component_diff_vars_regression(n_created, moments_fns=fns)
        R = fns[0].size
        assert means.shape == vars_.shape == (6, R) and l_vars.shape == reg.shape == (3, 6, R) and n_s.shape == (3, 6)
        assert n_s.dtype == np.int64
        assert np.all(means[:, 0] == 1.0) and np.all(vars_[:, 0] == 0.0)
        for m, (mean0, var0, l_vars0, n0, reg0, n_ops0) in enumerate(_loop(comps, st, fns, n_created)):
            assert np.array_equal(n_s[:, m], n0), (type(fns[0]).__name__, m)
            assert np.allclose(means[m], mean0, rtol=1e-10, atol=1e-14), (type(fns[0]).__name__, m)
            assert np.allclose(vars_[m], var0, rtol=1e-10, atol=0), (type(fns[0]).__name__, m)
            assert np.allclose(l_vars[:, m, :], l_vars0, rtol=1e-10, atol=0), (type(fns[0]).__name__, m)
            assert np.allclose(reg[:, m, :], reg0, rtol=1e-9, atol=0), (type(fns[0]).__name__, m)
            assert np.array_equal(n_ops, n_ops0)
        if isinstance(fns[0], Spline):                 # the loop route is the loop itself
            loop = _loop(comps, st, fns, n_created)
            assert np.array_equal(means, np.stack([r[0] for r in loop]))
            assert np.array_equal(l_vars, np.stack([r[2] for r in loop], axis=1))
        # two calls give the same bits
        means2, vars2 = est.estimate_component_moments(moments_fns=fns)
        l_vars2, n_s2 = est.estimate_component_diff_vars(moments_fns=fns)
        assert np.array_equal(means, means2) and np.array_equal(vars_, vars2)
        assert np.array_equal(l_vars, l_vars2, equal_nan=True) and np.array_equal(n_s, n_s2)
    # moments_fns=None: this Estimate's moments_fn for every component; a scalar quantity gives one row
    fn = Legendre(7, doms[0])
    means, vars_ = Estimate(root, st, fn).estimate_component_moments()
    assert means.shape == (6, 7)
    mean0, var0 = Estimate(comps[0], st, fn).estimate_moments()
    m1, v1 = Estimate(comps[0], st, fn).estimate_component_moments()
    assert m1.shape == v1.shape == (1, 7)
    assert np.allclose(m1[0], mean0, rtol=1e-10, atol=1e-14) and np.allclose(v1[0], var0, rtol=1e-10, atol=0)
    assert np.allclose(means[0], mean0, rtol=1e-10, atol=1e-14)


def test_all_masked_component_raises(hip):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    st, spec = _vector_storage(None)
    root, comps = _components(st, spec)
    doms = [Estimate.estimate_domain(q_m, st) for q_m in comps]
    fns = [Legendre(5, dom) for dom in doms]
    fns[3] = Legendre(5, (1e6, 2e6))                     # no sample of component 3 lies in this domain
    with pytest.raises(Exception, match="All samples were masked"):
        Estimate(root, st, fns[0]).estimate_component_moments(moments_fns=fns)
    with pytest.raises(Exception, match="All samples were masked"):
        Estimate(comps[3], st, fns[3]).estimate_moments()


def test_at_size_against_the_scalar_chain(hip):
    """M = 8, R = 64, 2.5 x 10^5 samples per level: several sample blocks per chunk and two term windows."""
    import torch
    from mlmc_amd import Legendre
    from mlmc_amd.engine import LevelAccumulator
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.sample_storage import Memory
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    from mlmc_amd.quantity.quantity import make_root_quantity
    from tests.util import level_arrays
    M, R, N = 8, 64, [250000, 220000, 200000]
    steps = [0.5, 0.07, 0.01]
    levels = level_arrays(N, steps, M, 0, seed=5)
    rng = np.random.default_rng(8)
    shift, scale = rng.normal(size=M), 0.5 + rng.random(M)
    data = []
    for f, c in levels:
        f = shift[:, None] + scale[:, None] * f
        c = None if c is None else shift[:, None] + scale[:, None] * c
        f[M - 1, 9::101] = np.nan
        data.append((f, c))
    spec = [QuantitySpec(name="q", unit="m", shape=(M, 1), times=[1], locations=['0'])]
    st = Memory(chunk_size=150000)
    st.save_global_data(result_format=spec, level_parameters=[[s] for s in steps])
    for l, (f, c) in enumerate(data):
        st.set_level_samples(l, f.T, None if c is None else c.T)
    root = make_root_quantity(st, spec)['q'][1]['0']
    doms = [(shift[m] - 3.0 * scale[m], shift[m] + 3.0 * scale[m]) for m in range(M)]
    fns = [Legendre(R, dom) for dom in doms]
    n, n_rm, s, sp = qe.component_level_sums(root, fns)
    for m in range(M):
        acc = LevelAccumulator(fns[m], len(N))
        for l, (f, c) in enumerate(data):
            acc.push(l, torch.from_numpy(f[m].copy()).cuda(), None if c is None else torch.from_numpy(c[m].copy()).cuda())
        n0, n_rm0, s0, sp0 = acc.finalize()
        assert np.array_equal(n[:, m], n0) and np.array_equal(n_rm[:, m], n_rm0), m
        sc = np.sqrt(np.abs(sp0) * n0[:, None]) + 1e-300
        assert np.all(np.abs(s[:, m, :] - s0) <= 1e-10 * np.maximum(np.abs(s0), sc)), m
        assert np.all(np.abs(sp[:, m, :] - sp0) <= 1e-10 * np.abs(sp0) + 1e-13), m


def _adaptive(component_call, n_levels=3):
    """The loop part of the reference's moments workflow (test_quantity_concept.py:526-575) on a 12-component quantity, one
    Legendre basis per component on its own domain.  -> (scheduled counts of every round, final n_estimated)"""
    from mlmc_amd import Legendre
    from mlmc_amd import estimator as est_mod
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.sampler import DeviceSampler
    from mlmc_amd.sim.synth_device import SynthDeviceStorage, result_format
    level_parameters = est_mod.determine_level_parameters(n_levels=n_levels, step_range=[0.5, 0.01])
    storage = SynthDeviceStorage(level_parameters, [0] * n_levels)
    sampler = DeviceSampler(storage, level_parameters)
    sampler.set_initial_n_samples([100, 60, 15])
    sampler.schedule_samples()
    sampler.ask_sampling_pool_for_samples()
    q = make_root_quantity(storage=storage, q_specs=result_format())['length']
    M = int(q.size())
    assert M == 12
    doms = est_mod.Estimate.estimate_domains(q, storage)
    fns = [Legendre(5, tuple(d)) for d in doms]
    target_var = 1e-3

    def n_estimated():
        variances, n_ops = component_call(q, storage, fns, sampler._n_scheduled_samples)
        return est_mod.estimate_n_samples_for_target_variance(target_var, variances.reshape(n_levels, -1), n_ops,
                                                              n_levels=sampler.n_levels)
    scheduled = [np.array(sampler._n_scheduled_samples).copy()]
    n_est = n_estimated()
    rounds = 0
    while not sampler.process_adding_samples(n_est, 0, 0.1):
        scheduled.append(np.array(sampler._n_scheduled_samples).copy())
        n_est = n_estimated()
        rounds += 1
        assert rounds < 200
    scheduled.append(np.array(sampler._n_scheduled_samples).copy())
    return scheduled, n_est


def test_adaptive_sample_allocation_loop_end_to_end(hip):
    from mlmc_amd import estimator as est_mod

    def batched(q, storage, fns, n_created):
        return est_mod.Estimate(q, storage, fns[0]).estimate_component_diff_vars_regression(n_created, moments_fns=fns)

    def loop(q, storage, fns, n_created):
        regs = []
        for m, fn in enumerate(fns):
            reg, n_ops = est_mod.Estimate(est_mod.scalar_component(q, m), storage, fn).estimate_diff_vars_regression(n_created)
            regs.append(reg)
        return np.stack(regs, axis=1), n_ops

    sched_a, n_a = _adaptive(batched)
    sched_b, n_b = _adaptive(loop)
    assert len(sched_a) == len(sched_b) and len(sched_a) > 2
    for a, b in zip(sched_a, sched_b):
        assert np.array_equal(a, b)
    assert np.array_equal(n_a, n_b)


def _both_entries(hip, fns, K, chunks):
    """mlmc_accum_estimate_multi and mlmc_accum_estimate_multi_var on the same bases and chunks [(level, fine [M, n], coarse [M, n]
    | None)], two levels -> (n, n_rm, sums), (n, n_rm, s, sp)"""
    lib, M, L = hip.lib(), len(fns), 2
    arr = (C.c_void_p * M)(*[fn._basis_handle().value for fn in fns])
    lv = np.array([c[0] for c in chunks], dtype=np.int32)
    nn = np.array([c[1].shape[1] for c in chunks], dtype=np.int64)
    fp = (C.c_void_p * len(chunks))(*[c[1].data_ptr() for c in chunks])
    cp = (C.c_void_p * len(chunks))(*[None if c[2] is None else c[2].data_ptr() for c in chunks])
    out = []
    for entry, n_float in ((lib.mlmc_accum_estimate_multi, 1), (lib.mlmc_accum_estimate_multi_var, 2)):
        n, n_rm = np.zeros((L, M), dtype=np.int64), np.zeros((L, M), dtype=np.int64)
        sums = [np.zeros((L, M, K)) for _ in range(n_float)]
        hip.check(entry(M, C.cast(arr, C.c_void_p), K, L, len(chunks), hip.ptr(lv), C.cast(fp, C.c_void_p), C.cast(cp, C.c_void_p),
                        hip.ptr(nn), hip.ptr(n), hip.ptr(n_rm), *[hip.ptr(v) for v in sums]))
        out.append((n, n_rm, *sums))
    return out


MEAN_ONLY_N = (1, 511, 512, 513, 4097)       # a single sample; the last trip of 2 x 256 lanes with and without its second
                                             # sample; two sample blocks


def _mean_only_data():
    """Per chunk length n: level 0 without coarse rows, level 1 in two chunks of n and 300 samples, M = 3.  Component 0: NaNs in
    its fine rows and values outside its domain (-2, 2); component 1: NaNs in its coarse rows, and not one value of its 300-sample
    chunk inside its domain; component 2: positive data (log=True)."""
    import torch
    rng = np.random.default_rng(2024)
    out = {}
    for n in MEAN_ONLY_N:
        chunks = []
        for level, length in ((0, n), (1, n), (1, 300)):
            f = rng.normal(size=(3, length))
            f[2] = np.exp(0.5 * f[2])
            c = f + 0.1 * rng.normal(size=f.shape)
            c[2] = f[2] * np.exp(0.05 * rng.normal(size=length))
            f[0, 3::7] = np.nan
            c[1, 2::5] = np.nan
            if length == 300:
                f[1] = 1e9
            chunks.append((level, torch.from_numpy(f).cuda(), None if level == 0 else torch.from_numpy(c).cuda()))
        out[n] = chunks
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def mean_only_chunks(hip):
    return _mean_only_data()


def _mean_only_fns(kind, K):
    from mlmc_amd import Legendre, Monomial, Fourier
    cls = {"legendre": Legendre, "monomial": Monomial, "fourier": Fourier}[kind]
    return [cls(K, (-2.0, 2.0)), cls(K, (-3.0, 3.5)), cls(K, (0.2, 6.0), log=True)]


MEAN_ONLY_CASES = [("legendre", 13), ("legendre", 25), ("legendre", 49), ("legendre", 97), ("monomial", 25), ("monomial", 49),
                   ("fourier", 25), ("fourier", 49)]


@pytest.mark.parametrize("kind,K", MEAN_ONLY_CASES)
def test_mean_only_entry_equals_the_variance_entry_bit_for_bit(hip, mean_only_chunks, kind, K):
    """Both C entries on the same bases and device chunks: equal counts, and the sums of the mean-only entry are the Σd of the
    variance entry, no tolerance.  K = 13: the 16-term tile; 25: one 32-term window with terms >= K discarded; 49: one window
    after the first; 97: windows that walk one and two 32-term blocks before their own."""
    fns = _mean_only_fns(kind, K)
    for n, chunks in mean_only_chunks.items():
        (n0, rm0, sums), (n1, rm1, s, sp) = _both_entries(hip, fns, K, chunks)
        assert np.array_equal(n0, n1) and np.array_equal(rm0, rm1), (kind, K, n)
        assert np.array_equal(sums, s), (kind, K, n, np.max(np.abs(sums - s)))
        # the cases are what they claim: every sample counted once, the 300-sample chunk of component 1 dropped whole, of
        # component 0 more than its NaNs dropped (the values outside its domain), finite sums
        assert np.array_equal(n1 + rm1, np.array([[n] * 3, [n + 300] * 3]))
        assert rm1[1, 1] >= 300 and rm1[1, 0] > len(range(3, n, 7)) + len(range(3, 300, 7))
        assert np.all(np.isfinite(s)) and np.all(np.isfinite(sp))


def test_abi_errors_name_the_component(hip):
    import torch
    from mlmc_amd import Legendre, Monomial
    from mlmc_amd.moments import TransformedMoments
    lib = hip.lib()
    M, n = 3, 100
    fine = torch.zeros((M, n), dtype=torch.float64, device="cuda")
    keep = []

    def call(fns, K, handles=None):
        hs = handles if handles is not None else [fn._basis_handle().value for fn in fns]
        arr = (C.c_void_p * len(hs))(*hs)
        lv = np.zeros(1, dtype=np.int32)
        nn = np.array([n], dtype=np.int64)
        fp = (C.c_void_p * 1)(fine.data_ptr())
        cp = (C.c_void_p * 1)(None)
        out_n = np.zeros((1, M), dtype=np.int64)
        out_rm = np.zeros((1, M), dtype=np.int64)
        s = np.zeros((1, M, max(K, 1)))
        sp = np.zeros((1, M, max(K, 1)))
        keep.append((arr, fp, cp))
        hip.check(lib.mlmc_accum_estimate_multi_var(M, C.cast(arr, C.c_void_p), K, 1, 1, hip.ptr(lv), C.cast(fp, C.c_void_p),
                                                    C.cast(cp, C.c_void_p), hip.ptr(nn), hip.ptr(out_n), hip.ptr(out_rm),
                                                    hip.ptr(s), hip.ptr(sp)))
        return out_n, s, sp
    dom = (-1.0, 1.0)
    out_n, s, sp = call([Legendre(4, dom)] * M, 4)
    assert np.array_equal(out_n, np.full((1, M), n)) and np.all(s[0, :, 0] == n) and np.all(sp[0, :, 0] == n)
    with pytest.raises(hip.MlmcHipError, match="mlmc_accum_estimate_multi_var: component 1: every component must use the same"):
        call([Legendre(4, dom), Monomial(4, dom), Legendre(4, dom)], 4)
    tm = TransformedMoments(Legendre(4, dom), np.eye(4))
    with pytest.raises(hip.MlmcHipError, match="component 2: transformed bases"):
        call([Legendre(4, dom), Legendre(4, dom), tm], 4)
    with pytest.raises(hip.MlmcHipError, match="component 0: basis smaller than K"):
        call([Legendre(4, dom)] * M, 5)
    for K in (0, 513):
        with pytest.raises(hip.MlmcHipError, match="mlmc_accum_estimate_multi_var: K must be in 1..512"):
            call([Legendre(4, dom)] * M, K)
    fn0 = Legendre(4, dom)
    handles = [fn0._basis_handle().value, None, None]
    with pytest.raises(hip.MlmcHipError, match="component 1: null basis"):
        call(None, 4, handles=handles)
    with pytest.raises(hip.MlmcHipError, match="null argument"):
        hip.check(lib.mlmc_accum_estimate_multi_var(M, None, 4, 1, 0, None, None, None, None, None, None, None, None))
