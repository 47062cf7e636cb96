"""Component covariance (mlmc_xcov_create, quantity_estimate.component_covariance, Estimate.estimate_component_covariance) on
the MI355X against the NumPy oracle: level sums of Y = (f - a)(f - a)^T - (c - a)(c - a)^T and of Y o Y, masking of whole
samples, chunking, shift, the Quantity API, the storages that feed it, and the errors it raises instead of faulting."""
import ctypes as C

import numpy as np
import pytest

from tests.util import close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


def _gram_ref(levels, shift):
    """Direct NumPy restatement over the kept samples: per level n, n_rm, s = sum Y, sp = sum Y o Y, and their scales
    sum (|f~_i f~_j| + |c~_i c~_j|) and sum (|f~_i f~_j| + |c~_i c~_j|)^2: the size of the terms Y is the difference of.
    (A sum of Y o Y is only as exact as its terms are large: one sample with Y_ij ~ 0 has a relative error of ~1 in Y_ij^2
    in any fp64 evaluation.)"""
    out = []
    for f, c in levels:
        M = f.shape[0]
        a = np.zeros(M) if shift is None else np.asarray(shift, dtype=np.float64)
        bad = np.isnan(f).any(axis=0) | (np.zeros(f.shape[1], bool) if c is None else np.isnan(c).any(axis=0))
        F = f[:, ~bad] - a[:, None]
        Cc = None if c is None else c[:, ~bad] - a[:, None]
        s = np.zeros((M, M))
        sp = np.zeros((M, M))
        sa = np.zeros((M, M))
        sq = np.zeros((M, M))
        b = max(1, (1 << 22) // (M * M))
        for k0 in range(0, F.shape[1], b):
            Fb = F[:, k0:k0 + b]
            Y = np.einsum("ik,jk->kij", Fb, Fb)
            A = np.abs(Y)
            if Cc is not None:
                Cb = Cc[:, k0:k0 + b]
                Z = np.einsum("ik,jk->kij", Cb, Cb)
                Y -= Z
                A += np.abs(Z)
            s += Y.sum(axis=0)
            sp += (Y * Y).sum(axis=0)
            sa += A.sum(axis=0)
            sq += (A * A).sum(axis=0)
        out.append((int(F.shape[1]), int(bad.sum()), s, sp, sa, sq))
    return out


def _outer_rows(shift):
    def rows(x):                                  # raw chunk [M, n, 2|1] -> rows [M * M, n, 2|1] (oracle operation node)
        M = x.shape[0]
        a = np.zeros(M) if shift is None else np.asarray(shift)
        y = x - a[:, None, None]
        return (y[:, None] * y[None, :]).reshape(M * M, x.shape[1], x.shape[2])
    return rows


def _levels(M, ns, seed, nan=True):
    """Components with different scales and correlations; NaN in different components of fine and coarse."""
    rng = np.random.default_rng(seed)
    mix = rng.normal(size=(M, M)) / np.sqrt(M)
    out = []
    for l, n in enumerate(ns):
        z = rng.normal(size=(M, n))
        f = mix @ z + np.linspace(-1.0, 2.0, M)[:, None] + 0.3 * rng.normal(size=(M, n))
        c = None if l == 0 else f + 0.2 * (mix @ rng.normal(size=(M, n)))
        if nan and n > 2:
            f[M // 2, 1::7] = np.nan
            if c is not None:
                c[M - 1, 2::11] = np.nan
                c[0, 5::13] = np.nan
        out.append((f, c))
    return out


def _acc_sums(levels, shift=None, mean_only=False, chunks=None, device=False):
    import torch
    from mlmc_amd.engine import ComponentCovAccumulator
    M = levels[0][0].shape[0]
    acc = ComponentCovAccumulator(M, len(levels), mean_only=mean_only)
    acc.set_shift(shift)
    for l, (f, c) in enumerate(levels):
        n = f.shape[1]
        cuts = [0, n] if chunks is None else sorted({0, n} | {int(x) for x in chunks(n) if 0 < x < n})
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            fb = np.ascontiguousarray(f[:, lo:hi])
            cb = None if c is None else np.ascontiguousarray(c[:, lo:hi])
            if device:
                fb = torch.from_numpy(fb).cuda()
                cb = None if cb is None else torch.from_numpy(cb).cuda()
            acc.push(l, fb, cb)
    out = acc.finalize()
    acc.close()
    return out


def _check(levels, shift, out, tol=1e-10):
    n, n_rm, s, sp = out
    L = len(levels)
    M = levels[0][0].shape[0]
    ref = _gram_ref(levels, shift)
    for l in range(L):
        rn, rrm, rs, rsp, rsa, rsq = ref[l]
        assert n[l] == rn and n_rm[l] == rrm, (l, n[l], rn, n_rm[l], rrm)
        S, SP = s[l].reshape(M, M), sp[l].reshape(M, M)
        assert np.array_equal(S, S.T) and np.array_equal(SP, SP.T, equal_nan=True)
        assert close(S, rs, scale=np.maximum(rsa, 1e-300), tol=tol), (l, np.max(np.abs(S - rs) / np.maximum(rsa, 1e-300)))
        assert close(SP, rsp, scale=np.maximum(rsq, 1e-300), tol=tol), (l, np.max(np.abs(SP - rsp) / np.maximum(rsq, 1e-300)))


@pytest.mark.parametrize("M", [1, 2, 15, 16, 17, 64, 65, 200, 1024])
def test_c_abi_sums_against_oracle(hip, M):
    if M == 1024:
        ns_list = [(0, 1, 3), (40, 3)]
    elif M >= 64:
        ns_list = [(4095, 1, 3, 0), (1000,)]
    else:
        ns_list = [(100000, 4095, 3, 1), (0, 4095), (1,)]
    for i, ns in enumerate(ns_list):
        levels = _levels(M, ns, seed=M * 10 + i)
        shift = None if i % 2 else np.linspace(0.5, -0.5, M)
        if sum(ns) == 0 or all(n == 0 for n in ns):
            continue
        _check(levels, shift, _acc_sums(levels, shift))
        # host vs device chunks: the same bits
        dev = _acc_sums(levels, shift, device=True)
        host = _acc_sums(levels, shift)
        assert all(np.array_equal(a, b) for a, b in zip(dev, host))


def test_c_abi_matches_oracle_estimate_mean(hip):
    """The oracle's own estimate_mean over the outer-product rows (quantity_estimate.py:22-80 with an operation node)."""
    from oracle import oracle_np as onp
    from tests.util import to_chunks
    for M, ns in ((5, (3000, 1500, 700, 64)), (33, (2000, 800))):
        levels = _levels(M, ns, seed=M)
        for shift in (None, np.linspace(1.0, 2.0, M)):
            n, n_rm, s, sp = _acc_sums(levels, shift)
            ref = onp.estimate_mean(to_chunks(levels), _outer_rows(shift))
            assert np.array_equal(n, ref.n_samples) and np.array_equal(n_rm, ref.n_rm_samples)
            scales = _gram_ref(levels, shift)
            for l in range(len(ns)):
                assert close(s[l], ref.sums[l], scale=scales[l][4].reshape(-1) + 1e-300)
                assert close(sp[l], ref.sums_sq[l], scale=scales[l][5].reshape(-1) + 1e-300)


def test_mean_only(hip):
    for M, ns in ((7, (5000, 3000)), (100, (2000, 999, 5))):
        levels = _levels(M, ns, seed=4)
        shift = np.full(M, 0.25)
        n, n_rm, s, sp = _acc_sums(levels, shift)
        n1, n_rm1, s1, sp1 = _acc_sums(levels, shift, mean_only=True)
        assert np.array_equal(n, n1) and np.array_equal(n_rm, n_rm1)
        assert np.all(np.isnan(sp1))
        ref = _gram_ref(levels, shift)
        for l in range(len(ns)):
            assert close(s1[l], s[l], scale=ref[l][4].reshape(-1) + 1e-300, tol=1e-12)
            assert np.array_equal(s1[l].reshape(M, M), s1[l].reshape(M, M).T)


def test_chunking_and_determinism(hip):
    for M in (9, 40, 130):
        levels = _levels(M, (20000, 7001, 333), seed=M + 1)
        whole = _acc_sums(levels)
        ragged = lambda n: [1, 2, 3, 17, 500, n // 3, n // 2 + 7, n - 1]   # noqa: E731
        a = _acc_sums(levels, chunks=ragged)
        b = _acc_sums(levels, chunks=ragged)
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
        assert np.array_equal(whole[0], a[0]) and np.array_equal(whole[1], a[1])
        ref = _gram_ref(levels, None)
        for l in range(3):
            assert close(a[2][l], whole[2][l], scale=ref[l][4].reshape(-1) + 1e-300)
            assert close(a[3][l], whole[3][l], scale=ref[l][5].reshape(-1) + 1e-300)


def test_shift_removes_cancellation(hip):
    rng = np.random.default_rng(11)
    M = 24
    mu = 1e6 + np.arange(M)
    levels = []
    for l, n in enumerate((30000, 8000, 2000)):
        f = mu[:, None] + rng.normal(size=(M, n))
        c = None if l == 0 else f + 0.1 * rng.normal(size=(M, n))
        levels.append((f, c))
    n, _, s, sp = _acc_sums(levels, mu)
    for l, (f, c) in enumerate(levels):
        F = f.astype(np.longdouble) - mu.astype(np.longdouble)[:, None]
        Y = np.einsum("ik,jk->kij", F, F)
        if c is not None:
            Cl = c.astype(np.longdouble) - mu.astype(np.longdouble)[:, None]
            Y = Y - np.einsum("ik,jk->kij", Cl, Cl)
        A = np.abs(np.einsum("ik,jk->kij", F, F))
        if c is not None:
            A = A + np.abs(np.einsum("ik,jk->kij", Cl, Cl))
        rs, rsp = Y.sum(axis=0), (Y * Y).sum(axis=0)
        assert np.all(np.abs(s[l].reshape(M, M) - rs) <= 1e-10 * A.sum(axis=0))
        assert np.all(np.abs(sp[l].reshape(M, M) - rsp) <= 1e-10 * (A * A).sum(axis=0))
    # raw mode (a = 0) against the unshifted oracle
    small = _levels(6, (3000, 900), seed=5)
    _check(small, None, _acc_sums(small, None))


def _zoo_storage(n=(700, 500, 300), chunk_size=None, nan=True):
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    from mlmc_amd.sample_storage import Memory
    from tests.zoo import level_data, result_format
    spec = result_format(QuantitySpec)
    st = Memory(chunk_size=chunk_size)
    st.save_global_data(result_format=spec, level_parameters=[[0.1], [0.01], [0.001]][:len(n)])
    rng = np.random.default_rng(21)
    for l, (f, c) in enumerate(level_data(n)):
        f = f.copy()
        f[:, :12] = f[:, :12] @ (np.eye(12) + 0.3 * rng.normal(size=(12, 12)))    # genuinely different, correlated components
        if c is not None:
            c = f + 0.1 * rng.normal(size=f.shape)
        if nan:
            f[3::97, 5] = np.nan
            if c is not None:
                c[10::89, 2] = np.nan
        st.set_level_samples(l, f, c)
    return st, spec


def _quantity_chunks(q):
    qs = q.get_quantity_storage()
    by_level = {}
    for cs in qs.chunks():
        by_level.setdefault(int(cs.level_id), []).append(np.asarray(q.samples(cs)))
    return [by_level[l] for l in sorted(by_level)]


def test_api_parity_with_oracle_and_tree_route(hip):
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.quantity.quantity import make_root_quantity
    from oracle import oracle_np as onp
    st, spec = _zoo_storage()
    q = make_root_quantity(st, spec)['length']
    M = int(q.size())
    assert M == 12
    chunks = _quantity_chunks(q)
    for shift in (None, np.linspace(1.0, 3.0, M)):
        r = qe.estimate_mean(qe.component_covariance(q, shift))
        ref = onp.estimate_mean(chunks, _outer_rows(shift))
        assert np.array_equal(r.n_samples, ref.n_samples) and np.array_equal(r.n_rm_samples, ref.n_rm_samples)
        assert r.mean.shape == (M, M)
        assert close(r.l_means.reshape(len(chunks), -1), np.array(ref.l_means), scale=1e-12)
        assert close(r.l_vars.reshape(len(chunks), -1), np.array(ref.l_vars), scale=1e-12)
    # the reference's route: one derived quantity per pair (a = 0).  It masks a sample only for a NaN in q_i or q_j, the
    # component covariance for a NaN anywhere in the vector: compared on samples without NaN
    st, spec = _zoo_storage(nan=False)
    q = make_root_quantity(st, spec)['length']
    r = qe.estimate_mean(qe.component_covariance(q))
    flat = [q[t][loc][i, 0] for t in (1, 2, 3) for loc in ('10', '20') for i in range(2)]
    for i, j in ((0, 0), (0, 5), (3, 11), (7, 2)):
        p = qe.estimate_mean(flat[i] * flat[j])
        assert list(p.n_samples) == list(r.n_samples)
        assert close(r.mean[i, j], p.mean.reshape(()), scale=1e-12)
        assert close(r.var[i, j], p.var.reshape(()), scale=1e-20)
        assert close(r.l_means[:, i, j], p.l_means.reshape(-1), scale=1e-12)
        assert close(r.l_vars[:, i, j], p.l_vars.reshape(-1), scale=1e-20)


def test_estimate_component_covariance(hip):
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    from mlmc_amd.sample_storage import Memory
    from mlmc_amd.quantity import quantity_estimate as qe
    from oracle import oracle_np as onp
    # one level: np.cov(bias=True) of the kept samples
    levels = _levels(10, (5000,), seed=8)
    f = levels[0][0]
    spec = [QuantitySpec(name="q", unit="m", shape=(5, 1), times=[1, 2], locations=['0'])]
    st = Memory()
    st.save_global_data(result_format=spec, level_parameters=[[0.1]])
    st.set_level_samples(0, f.T)
    q = make_root_quantity(st, spec)['q']
    chunks = _quantity_chunks(q)
    X = chunks[0][0][:, :, 0]
    keep = ~np.isnan(X).any(axis=0)
    cov, cov_var = Estimate(q, st).estimate_component_covariance()
    ref = np.cov(X[:, keep], bias=True)
    assert close(cov, ref, scale=np.abs(ref).max() * 1e-3)
    raw, _ = Estimate(q, st).estimate_component_covariance(centered=False)
    assert close(raw, X[:, keep] @ X[:, keep].T / keep.sum(), scale=1e-12)
    # several levels: the oracle plug-in with a = the MLMC mean; cov_var = sum_l l_vars / n_l
    st, spec = _zoo_storage()
    q = make_root_quantity(st, spec)['length']
    M = int(q.size())
    chunks = _quantity_chunks(q)
    a = np.sum(np.array(onp.estimate_mean(chunks).l_means), axis=0).reshape(M)
    cov, cov_var = Estimate(q, st).estimate_component_covariance()
    ref = onp.estimate_mean(chunks, _outer_rows(a))
    ref_cov = np.sum(np.array(ref.l_means), axis=0).reshape(M, M)
    assert close(cov, ref_cov, scale=np.abs(ref_cov).max() * 1e-6)
    r = qe.estimate_mean(qe.component_covariance(q, np.asarray(qe.estimate_mean(q).mean).reshape(M)))
    assert np.array_equal(cov, r.mean) and np.array_equal(cov_var, r.var)
    n = np.asarray(r.n_samples, dtype=np.float64)
    assert close(cov_var, np.sum(r.l_vars / n[:, None, None], axis=0), scale=1e-300, tol=1e-14)
    assert np.array_equal(cov, cov.T)


def test_feeds_and_sharding(hip):
    import torch
    from mlmc_amd import _lib
    from mlmc_amd.engine import ComponentCovAccumulator, unpack_partials
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.sample_storage import DeviceMemory
    n = (4000, 2500, 1200)
    results = []
    for chunk_size in (None, 333):
        st, spec = _zoo_storage(n, chunk_size=chunk_size)
        qe.device_cache_clear()
        q = make_root_quantity(st, spec)['length']
        results.append(qe.estimate_mean(qe.component_covariance(q, np.full(12, 2.0))))
        results.append(qe.estimate_mean(qe.component_covariance(q, np.full(12, 2.0))))    # resident cache
    st, spec = _zoo_storage(n)
    host_q = make_root_quantity(st, spec)['length']
    chunks = _quantity_chunks(host_q)
    dev = DeviceMemory()
    dev.save_global_data(result_format=spec, level_parameters=[[0.1], [0.01], [0.001]])
    full = _zoo_full_levels(st)
    for l, pairs in enumerate(full):
        dev.set_level_samples(l, torch.from_numpy(pairs).cuda())
    qe.device_cache_clear()
    results.append(qe.estimate_mean(qe.component_covariance(make_root_quantity(dev, spec)['length'], np.full(12, 2.0))))
    base = results[0]
    for r in results[1:]:
        assert list(r.n_samples) == list(base.n_samples) and list(r.n_rm_samples) == list(base.n_rm_samples)
        assert close(r.l_means, base.l_means, scale=1e-12)
        assert close(r.l_vars, base.l_vars, scale=1e-20)
    # two half shards' packed partial sums, added on the host, equal the whole estimate
    levels = [(x[:, :, 0].copy(), None if l == 0 else x[:, :, 1].copy()) for l, x in enumerate(c[0] for c in chunks)]
    whole = _acc_sums(levels)
    packed = []
    for half in (0, 1):
        acc = ComponentCovAccumulator(12, 3)
        for l, (f, c) in enumerate(levels):
            m = f.shape[1] // 2
            sl = slice(0, m) if half == 0 else slice(m, None)
            acc.push(l, np.ascontiguousarray(f[:, sl]), None if c is None else np.ascontiguousarray(c[:, sl]))
        buf = np.empty(2 * 3 + 2 * 3 * 144)
        _lib.check(_lib.lib().mlmc_accum_finalize_packed(acc._h, _lib.ptr(buf), _lib.HOST))
        packed.append(buf)
        acc.close()
    nn, nrm, s, sp = unpack_partials(packed[0] + packed[1], 3, 144)
    assert np.array_equal(nn, whole[0]) and np.array_equal(nrm, whole[1])
    assert close(s, whole[2], scale=np.abs(whole[2]).max() * 1e-12) and close(sp, whole[3], scale=1e-300)


def _zoo_full_levels(st):
    """[M_stored, n, 2] per level of the host storage (DeviceMemory's layout)."""
    from mlmc_amd.sample_storage import ChunkSpec
    return [np.ascontiguousarray(st.sample_pairs_level(ChunkSpec(level_id=l))) for l in range(3)]


def test_subsample(hip):
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.quantity.quantity import make_root_quantity
    st, spec = _zoo_storage((3000, 2000, 1000))
    q = make_root_quantity(st, spec)['length']
    sub = q.subsample(sample_vec=[500, 300, 100])
    r = qe.estimate_mean(qe.component_covariance(sub))
    assert np.sum(r.n_samples + r.n_rm_samples) == 900
    assert r.mean.shape == (12, 12) and np.array_equal(r.mean, r.mean.T)


def test_errors_not_faults(hip):
    from mlmc_amd import _lib
    from mlmc_amd.engine import ComponentCovAccumulator
    acc = ComponentCovAccumulator(4, 2)
    with pytest.raises(ValueError, match="components"):
        acc.push(0, np.zeros((3, 10)))
    acc.push(0, np.ones((4, 10)))
    with pytest.raises(_lib.MlmcHipError, match="pending"):
        acc.set_shift(np.zeros(4))
    acc.reset()
    acc.set_shift(np.ones(4))
    with pytest.raises(ValueError, match="shape"):
        acc.set_shift(np.ones(5))
    acc.push(1, np.ones((4, 10)), np.ones((4, 10)))
    n, n_rm, s, sp = acc.finalize()
    assert list(n) == [0, 10] and not np.any(s) and not np.any(sp)
    acc.close()
    h = C.c_void_p()
    assert _lib.lib().mlmc_xcov_create(1025, 2, 0, C.byref(h)) != 0
    assert "1024" in _lib.lib().mlmc_last_error().decode()
    assert _lib.lib().mlmc_xcov_create(8, 2, 0x1, C.byref(h)) != 0
    with pytest.raises(ValueError, match="1024"):
        ComponentCovAccumulator(1025, 2)
