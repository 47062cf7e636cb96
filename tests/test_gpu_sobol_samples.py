"""GPU tests of the scrambled Sobol' draws (MLMC_SAMPLE_SOBOL; the QMC instances of k_q_sample in mlmc_amd/csrc/density.hip and
k_cop_sobol_normals in sobol.hip) through mlmc_density_sample_batch, mlmc_density_sample_joint_batch,
mlmc_density_sample_conditional_batch and the Python entries with qmc=True.

The uniforms are compared bit for bit with their NumPy restatement (tests/sobol_cases.py), the draws bit for bit with
mlmc_density_quantiles_batch at the returned uniforms, the normals with mpmath at the restatement's uniforms under the tolerance of
the Philox normals, the structure bit for bit, and the error of two integrals with the error of the same entry without the flag."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import joint_sample_cases as jc
from tests import sobol_cases as sb
from tests.test_gpu_conditional_samples import _cok, _cond
from tests.test_gpu_density_samples import SEED, _call, _quantiles_c, _same, _small_vector_storage
from tests.test_gpu_joint_samples import _cycle, _joint, _ok, hip, table  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
SOBOL = 8                                            # MLMC_SAMPLE_SOBOL
DIMS = [0, 1, 7, 1023]
FIRSTS = (0, 1, 4095, 2 ** 20 + 3, 2 ** 40 + 5)
N = 1000                                             # no multiple of a workgroup, a wave or a block of draws
STREAMS5 = [0, 7, 1023, 11, 3]


def _want_uniforms(seed, dims, first, n):
    return np.concatenate([sb.uniforms(seed, d, f, k) for d, f, k in zip(dims, first, n)] + [np.zeros(0)])


@pytest.mark.parametrize("first", FIRSTS)
def test_marginal_uniforms_and_inversion(hip, table, first):
    """u_out == the restatement and out == mlmc_density_quantiles_batch(u_out), bit for bit: dimensions 0, 1, 7 and 1023, n = 1000,
    host and device arrays, with and without u_out; on both rules (the second stages no P row of this length differently)"""
    for group6 in table:
        group, quad = group6[:4], group6[0]["quad"]
        want_u = _want_uniforms(SEED, DIMS, [first] * 4, [N] * 4)
        assert np.all((want_u > 0) & (want_u < 1))
        rc, out, u, mass = _call(hip, group, quad, [N] * 4, SEED, DIMS, [first] * 4, flags=SOBOL, want_mass=True)
        hip.check(rc)
        assert _same(u, want_u), quad
        want, want_mass = _quantiles_c(hip, group, quad, u, [N] * 4)
        assert _same(out, want) and np.array_equal(mass, want_mass) and np.all(np.isfinite(out)), quad
        rc, out_d, u_d, _ = _call(hip, group, quad, [N] * 4, SEED, DIMS, [first] * 4, flags=SOBOL, kind=hip.DEVICE)
        hip.check(rc)
        assert _same(u_d, want_u) and _same(out_d, want), quad
        for kind in (hip.HOST, hip.DEVICE):
            rc, out_n, u_n, _ = _call(hip, group, quad, [N] * 4, SEED, DIMS, [first] * 4, flags=SOBOL, kind=kind, want_u=False)
            hip.check(rc)
            assert u_n is None and _same(out_n, want), (quad, kind)


def test_marginal_independence(hip, table):
    """first = 50, n = 100 == [50, 150) of n = 150; a problem alone == anywhere in a batch, in any order; default streams are the
    problems' indices; equal streams share their uniforms; other launch geometries; another seed gives other points"""
    rng = np.random.default_rng(3)
    group = table[0]
    quad, B = group[0]["quad"], len(group)
    dims = np.array([5, 0, 1023, 11, 11, 7])
    rc, whole, whole_u, _ = _call(hip, group, quad, [150] * B, SEED, dims, flags=SOBOL)
    hip.check(rc)
    assert _same(whole_u, _want_uniforms(SEED, dims, [0] * B, [150] * B))
    rc, part, part_u, _ = _call(hip, group, quad, [100] * B, SEED, dims, [50] * B, flags=SOBOL)
    hip.check(rc)
    whole, whole_u = whole.reshape(B, 150), whole_u.reshape(B, 150)
    assert _same(part.reshape(B, 100), whole[:, 50:]) and _same(part_u.reshape(B, 100), whole_u[:, 50:])
    assert _same(whole_u[3], whole_u[4]) and not _same(whole_u[0], whole_u[1])
    perm = rng.permutation(B)
    rc, shuffled, shuffled_u, _ = _call(hip, [group[i] for i in perm], quad, [150] * B, SEED, dims[perm], flags=SOBOL)
    hip.check(rc)
    assert _same(shuffled.reshape(B, 150), whole[perm]) and _same(shuffled_u.reshape(B, 150), whole_u[perm])
    for k in (0, B - 1):
        rc, alone, _, _ = _call(hip, [group[k]], quad, [150], SEED, [dims[k]], flags=SOBOL)
        assert rc == 0 and _same(alone, whole[k]), group[k]["tag"]
    rc, _, default_u, _ = _call(hip, group, quad, [64] * B, SEED, flags=SOBOL)
    hip.check(rc)
    assert _same(default_u, _want_uniforms(SEED, range(B), [0] * B, [64] * B))
    # 300 copies of a problem (more workgroups), mixed counts with an empty problem, and 70000 draws of one problem (several
    # workgroups in y, lists of several draws per lane)
    rc, copies, _, _ = _call(hip, [group[0]] * 300, quad, [150] * 300, SEED, [dims[0]] * 300, flags=SOBOL, want_u=False)
    assert rc == 0 and _same(copies.reshape(300, 150), np.tile(whole[0], (300, 1)))
    rc, big, big_u, _ = _call(hip, group[:4], quad, [2, 70000, 0, 150], SEED, dims[:4], flags=SOBOL)
    assert rc == 0 and _same(big[:2], whole[0, :2]) and _same(big[2:152], whole[1]) and _same(big[70002:], whole[3])
    assert _same(big_u[2:70002], sb.uniforms(SEED, 0, 0, 70000))
    assert _same(big[2:70002], _quantiles_c(hip, [group[1]], quad, big_u[2:70002], [70000])[0])
    rc, _, other_u, _ = _call(hip, group, quad, [150] * B, SEED + 1, dims, flags=SOBOL)
    assert rc == 0 and not _same(other_u.reshape(B, 150)[0], whole_u[0])
    # the points are balanced: 4096 draws from a multiple of 4096 hit every stratum once
    rc, _, u, _ = _call(hip, group[:1], quad, [4096], SEED, [1023], [3 * 4096], flags=SOBOL)
    assert rc == 0 and np.array_equal(np.sort(np.floor(u * 4096).astype(np.int64)), np.arange(4096))


@pytest.mark.parametrize("K", [1, 3, 5])
def test_joint_normals(hip, table, K):
    """z_out against mpmath at the restatement's uniforms, the comparison and tolerance of the Philox normals
    (test_gpu_joint_samples.py::test_normals): K latent normals, n = 257 from first = 2^20 + 3, default and explicit dimensions"""
    n, first = 257, 2 ** 20 + 3
    for streams in (None, STREAMS5[:K]):
        dims = list(range(K)) if streams is None else streams
        for kind in (hip.HOST, hip.DEVICE):
            _, u, z, _ = _ok(hip, _cycle(table[0], K), np.eye(K), n, streams=streams, first=first, flags=SOBOL, kind=kind)
            u0 = sb.latent_uniforms(SEED, dims, first, n)
            assert z.shape == (K, n) and np.all(np.isfinite(z))
            units = jc.z_units(z, jc.mp_ndtri(u0))
            k = int(np.argmax(units))
            print(f"\nK {K} dims {dims}: worst {units[k]:.4g} units at u0 = {u0.ravel()[k]!r} (tolerance {jc.z_tolerance():g})")
            assert units[k] <= jc.z_tolerance()
            # F = I: u = clamp(Phi(z)) returns to the point within phi(z) |dz| + E_Phi 2^-53 u with |dz| <= 16 2^-53 max(1, |z|)
            # (z_tolerance) and phi(z) max(1, |z|) <= 0.4: 6.4 + 16 units of 2^-53, far from another point of the sequence
            assert np.all(np.abs(u - u0) <= 64 * jc.U)


def test_joint_structure_and_inversion(hip, table):
    """u_out and x do not depend on M, on the row's position or on the block length of the draws; x is the quantile entry at
    u_out; continuation; equal dimensions give equal normals; host and device arrays"""
    rng = np.random.default_rng(11)
    M, K, n, first = 65, 5, 257, 3
    group = _cycle(table[1], M)
    quad = group[0]["quad"]
    F = jc.random_factor(rng, M, K)
    whole = _ok(hip, group, F, n, first=first, streams=STREAMS5, flags=SOBOL, want_mass=True)
    out, u, z, mass = whole
    assert _same(z, _ok(hip, group[:5], np.eye(5), n, first=first, streams=STREAMS5, flags=SOBOL)[2])
    want, want_mass = _quantiles_c(hip, group, quad, u.ravel(), [n] * M)
    assert _same(out.ravel(), want) and np.array_equal(mass, want_mass) and np.all(np.isfinite(out))
    for m in (0, 16, 63, 64):
        alone = _ok(hip, [group[m]], F[m:m + 1], n, first=first, streams=STREAMS5, flags=SOBOL)
        assert _same(alone[0][0], out[m]) and _same(alone[1][0], u[m]) and _same(alone[2], z), m
    perm = rng.permutation(M)
    moved = _ok(hip, [group[i] for i in perm], F[perm], n, first=first, streams=STREAMS5, flags=SOBOL)
    assert _same(moved[0], out[perm]) and _same(moved[1], u[perm]) and _same(moved[2], z)
    part = _ok(hip, group, F, 100, first=first + 50, streams=STREAMS5, flags=SOBOL)
    assert _same(part[0], out[:, 50:150]) and _same(part[1], u[:, 50:150]) and _same(part[2], z[:, 50:150])
    dev = _ok(hip, group, F, n, first=first, streams=STREAMS5, flags=SOBOL, kind=hip.DEVICE)
    assert all(_same(g, w) for g, w in zip(dev[:3], whole[:3]))
    assert _same(_ok(hip, group, F, n, first=first, streams=STREAMS5, flags=SOBOL, kind=hip.DEVICE, want_u=False, want_z=False)[0], out)
    twice = _ok(hip, group[:2], jc.random_factor(rng, 2, 3), 64, streams=[9, 4, 9], flags=SOBOL)[2]
    assert _same(twice[0], twice[2]) and not _same(twice[0], twice[1])
    assert "MLMC_JOINT_BLOCK_DRAWS" not in os.environ
    try:
        for block in ("64", "192"):
            os.environ["MLMC_JOINT_BLOCK_DRAWS"] = block
            for kind in (hip.HOST, hip.DEVICE):
                got = _ok(hip, group, F, n, first=first, streams=STREAMS5, flags=SOBOL, kind=kind)
                assert all(_same(g, w) for g, w in zip(got[:3], whole[:3])), (block, kind)
        ms, launches = C.c_double(), C.c_int64()
        hip.check(hip.lib().mlmc_density_quantiles_kernel_time(C.byref(ms), C.byref(launches)))
        _ok(hip, group, F, n, flags=SOBOL)
        hip.check(hip.lib().mlmc_density_quantiles_kernel_time(C.byref(ms), C.byref(launches)))
        assert launches.value == 2 and ms.value > 0              # one per block of 192
    finally:
        del os.environ["MLMC_JOINT_BLOCK_DRAWS"]


def test_conditional_structure(hip, table):
    """a zero shift with unit rows gives the joint entry's bits; a set does not depend on B or on its position, nor on the block
    length; x is the quantile entry at u_out"""
    rng = np.random.default_rng(21)
    M, K, n, B, first = 17, 5, 257, 4, 2 ** 20 + 3
    group = _cycle(table[0], M)
    quad = group[0]["quad"]
    F = jc.random_factor(rng, M, K)
    want = _ok(hip, group, F, n, first=first, streams=STREAMS5, flags=SOBOL)[:3]
    for shift in (None, np.zeros((1, M))):
        for kind in (hip.HOST, hip.DEVICE):
            out, u, z, _ = _cok(hip, group, F, n, first=first, streams=STREAMS5, shift=shift, flags=SOBOL, kind=kind)
            assert _same(out[0], want[0]) and _same(u[0], want[1]) and _same(z, want[2]), (shift is None, kind)
    Fc = F * rng.uniform(0.2, 1.0, M)[:, None]
    shift = rng.uniform(-3.0, 3.0, (B, M))
    out, u, z, mass = _cok(hip, group, Fc, n, B=B, shift=shift, first=first, streams=STREAMS5, flags=SOBOL, want_mass=True)
    assert _same(z, want[2])
    got, got_mass = _quantiles_c(hip, group * B, quad, u.ravel(), [n] * (M * B))
    assert _same(out.ravel(), got) and np.array_equal(np.tile(mass, B), got_mass)
    for b in (0, B - 1):
        alone = _cok(hip, group, Fc, n, B=1, shift=shift[b:b + 1], first=first, streams=STREAMS5, flags=SOBOL)
        assert _same(alone[0][0], out[b]) and _same(alone[1][0], u[b]), b
    order = rng.permutation(B)
    moved = _cok(hip, group, Fc, n, B=B, shift=shift[order], first=first, streams=STREAMS5, flags=SOBOL)
    assert _same(moved[0], out[order]) and _same(moved[1], u[order])
    fewer = _cok(hip, group[3:9], Fc[3:9], n, B=B, shift=shift[:, 3:9], first=first, streams=STREAMS5, flags=SOBOL)
    assert _same(fewer[0], out[:, 3:9]) and _same(fewer[1], u[:, 3:9])
    assert "MLMC_JOINT_BLOCK_DRAWS" not in os.environ
    try:
        for block in ("64", "192"):
            os.environ["MLMC_JOINT_BLOCK_DRAWS"] = block
            for kind in (hip.HOST, hip.DEVICE):
                blocked = _cok(hip, group, Fc, n, B=B, shift=shift, first=first, streams=STREAMS5, flags=SOBOL, kind=kind)
                assert _same(blocked[0], out) and _same(blocked[1], u) and _same(blocked[2], z), (block, kind)
    finally:
        del os.environ["MLMC_JOINT_BLOCK_DRAWS"]


def test_long_runs(hip, table):
    """2^20 + 5 draws of one problem and 300 001 joint draws of three: every lane owns a run of several consecutive draws and steps
    from one point to the next by its Gray code; the uniforms are still the restatement's, the draws the quantile entry's at them
    (compared on the device), and neither depends on the block length, which changes the runs"""
    import torch
    from mlmc_amd.tool import simple_distribution as sd
    distrs = [p["dist"] for p in table[0][:3]]
    n, first = 2 ** 20 + 5, 2 ** 40 + 5
    x, u = sd.samples(distrs[:1], n, SEED, streams=[7], first=first, device=True, return_uniforms=True, qmc=True)
    assert _same(u[0].cpu().numpy(), sb.uniforms(SEED, 7, first, n))
    assert torch.equal(x[0], sd.quantiles(distrs[:1], u)[0]) and bool(torch.isfinite(x[0]).all())
    n = 300_001
    F, _ = sd.correlation_factor(jc.CORR3)
    x, u, z = sd.joint_samples(distrs, n, SEED, factor=F, first=first, device=True, return_uniforms=True, return_normals=True, qmc=True)
    tail = jc.z_units(z[:, -300:].cpu().numpy(), jc.mp_ndtri(sb.latent_uniforms(SEED, range(3), first + n - 300, 300)))
    assert np.max(tail) <= jc.z_tolerance()
    want = sd.quantiles(distrs, list(u))
    assert all(torch.equal(a, b) for a, b in zip(x, want))
    assert "MLMC_JOINT_BLOCK_DRAWS" not in os.environ
    os.environ["MLMC_JOINT_BLOCK_DRAWS"] = "65536"
    try:
        xb, ub, zb = sd.joint_samples(distrs, n, SEED, factor=F, first=first, device=True, return_uniforms=True, return_normals=True,
                                      qmc=True)
    finally:
        del os.environ["MLMC_JOINT_BLOCK_DRAWS"]
    assert torch.equal(xb, x) and torch.equal(ub, u) and torch.equal(zb, z)
    x1 = sd.quantiles([distrs[1]], [np.array([0.2, 0.93])])[0]
    xc, uc = sd.conditional_samples(distrs, 150_001, SEED, {1: x1}, corr=jc.CORR3, first=first, device=True, return_uniforms=True,
                                    qmc=True)
    for b in range(2):
        want = sd.quantiles([distrs[0], distrs[2]], [uc[b, 0], uc[b, 2]])
        assert torch.equal(xc[b, 0], want[0]) and torch.equal(xc[b, 2], want[1])
    small, _ = sd.conditional_samples(distrs, 257, SEED, {1: x1}, corr=jc.CORR3, first=first + 150_001 - 257, return_uniforms=True, qmc=True)
    assert _same(xc[:, :, -257:].cpu().numpy(), small)


def test_errors(hip, table):
    """both flags, a stream of 1024, first + n = 2^52 + 1 and the unknown bits 2 and 4, on the three entries"""
    group = list(table[0][:3])
    quad = group[0]["quad"]
    F = np.eye(3)

    def expect(rc, pattern):
        with pytest.raises(hip.MlmcHipError, match=pattern):
            hip.check(rc)
    name = "mlmc_density_sample_batch"
    assert _call(hip, group, quad, [2, 2, 2], 1, flags=SOBOL)[0] == 0
    expect(_call(hip, group, quad, [2, 2, 2], 1, flags=SOBOL | 1)[0], name + ": MLMC_SAMPLE_SOBOL and MLMC_SAMPLE_ANTITHETIC")
    expect(_call(hip, group, quad, [2, 2, 2], 1, [0, 1024, 1], flags=SOBOL)[0], name + ": problem 1: stream 1024")
    assert _call(hip, group, quad, [2, 2, 2], 1, [0, 1023, 1], flags=SOBOL)[0] == 0
    assert _call(hip, group, quad, [2, 2, 2], 1, [0, 1024, 1])[0] == 0                       # a Philox stream
    expect(_call(hip, group, quad, [2, 2, 2], 1, first=[0, 0, 2 ** 52 - 1], flags=SOBOL)[0], name + ": problem 2.*2\\^52")
    assert _call(hip, group, quad, [2, 2, 2], 1, first=[0, 0, 2 ** 52 - 2], flags=SOBOL)[0] == 0
    expect(_call(hip, group, quad, [2, 2, 2], 1, flags=SOBOL | 4)[0], name + ": unknown flag")
    expect(_call(hip, group, quad, [2, 2, 2], 1, flags=4)[0], name + ": unknown flag")
    expect(_call(hip, group, quad, [2, 2, 2], 1, flags=SOBOL | 2)[0], name + ": unknown flag")
    rc, last, last_u, _ = _call(hip, group[:1], quad, [2], 1, [7], first=[2 ** 52 - 2], flags=SOBOL)
    assert rc == 0 and _same(last_u, sb.uniforms(1, 7, 2 ** 52 - 2, 2))
    for name, call in (("mlmc_density_sample_joint_batch", lambda **kw: _joint(hip, group, F, 2, **kw)[0]),
                       ("mlmc_density_sample_conditional_batch", lambda **kw: _cond(hip, group, F, 2, **kw)[0])):
        assert call(flags=SOBOL) == 0
        expect(call(flags=SOBOL | 1), name + ": MLMC_SAMPLE_SOBOL and MLMC_SAMPLE_ANTITHETIC")
        expect(call(flags=SOBOL, streams=[0, 1, 1024]), name + ": latent normal 2: stream 1024")
        assert call(flags=SOBOL, streams=[0, 1, 1023]) == 0
        assert call(streams=[0, 1, 1024]) == 0
        expect(call(flags=SOBOL, first=2 ** 52 - 1), name + ".*2\\^52")
        assert call(flags=SOBOL, first=2 ** 52 - 2) == 0
        expect(call(flags=SOBOL | 4), name + ": unknown flag")
        expect(call(flags=4), name + ": unknown flag")
        expect(call(flags=SOBOL | 2), name + ": unknown flag")


def _rms_errors(hip, group, F, g, exact, flags):
    err = []
    for seed in range(1, 9):
        _, u, _, _ = _ok(hip, group, F, 4096, seed=seed, flags=flags, want_z=False)
        err.append(float(np.mean(g(u))) - exact)
    return float(np.sqrt(np.mean(np.square(err))))


def test_accuracy(hip, table):
    """RMS error over seeds 1 .. 8 of the mean of g(u_out) at n = 4096 from the joint entry: with the flag it is at most 1 / 20 of the
    error without it, for g = prod_m (1 + 0.8 (u_m - 1/2)) under M = K = 4, F = I (exact mean 1) and for g = u_0 u_1 under the
    correlation CORR3 (exact mean 1/4 + arcsin(rho_01 / 2) / (2 pi)).  On the restatement alone (NumPy, scipy's ndtr / ndtri) the
    ratios at n = 4096 are 1 / 500 and 1 / 278, so n = 4096 stands for the second integral too."""
    from mlmc_amd.tool import simple_distribution as sd
    print()
    cases = (("product of 4", _cycle(table[0], 4), np.eye(4), lambda u: np.prod(1.0 + 0.8 * (u - 0.5), axis=0), 1.0),
             ("u0 u1 under CORR3", _cycle(table[0], 3), sd.correlation_factor(jc.CORR3)[0], lambda u: u[0] * u[1],
              0.25 + float(np.arcsin(jc.CORR3[0, 1] / 2.0)) / (2.0 * np.pi)))
    for tag, group, F, g, exact in cases:
        qmc = _rms_errors(hip, group, F, g, exact, SOBOL)
        plain = _rms_errors(hip, group, F, g, exact, 0)
        print(f"{tag}: RMS error {qmc:.3g} with the flag, {plain:.3g} without, ratio 1 / {plain / qmc:.0f}")
        assert qmc <= plain / 20.0, tag


def test_python_entries(hip, table):
    """samples, joint_samples, conditional_samples and rvs with qmc=True return what the C entries return with the flag"""
    import torch
    from mlmc_amd.tool import simple_distribution as sd
    from mlmc_amd.tool.distribution import Distribution
    from tests.test_gpu_quantiles import _dist
    group = table[1][:3]
    quad = group[0]["quad"]
    distrs = [p["dist"] for p in group]
    first = 2 ** 20 + 3
    rc, want, want_u, _ = _call(hip, group, quad, [257] * 3, SEED, [7, 0, 1023], [first] * 3, flags=SOBOL)
    hip.check(rc)
    xs, us = sd.samples(distrs, 257, SEED, streams=[7, 0, 1023], first=first, qmc=True, return_uniforms=True)
    assert _same(np.concatenate(xs), want) and _same(np.concatenate(us), want_u)
    assert not _same(np.concatenate(sd.samples(distrs, 257, SEED, streams=[7, 0, 1023], first=first)), want)
    dev = sd.samples(distrs, 257, SEED, streams=[7, 0, 1023], first=first, qmc=True, device=True)
    assert all(isinstance(d, torch.Tensor) and d.is_cuda for d in dev) and _same(torch.cat(dev).cpu().numpy(), want)
    assert _same(distrs[2].rvs(257, SEED, stream=1023, first=first, qmc=True), xs[2])
    old = _dist(group[0]["case"], group[0]["lam"], quad, Distribution)
    assert _same(old.rvs(257, SEED, stream=7, first=first, qmc=True), xs[0])
    assert _same(sd.samples(distrs, 64, SEED, qmc=True, return_uniforms=True)[1][2], sb.uniforms(SEED, 2, 0, 64))
    F, _ = sd.correlation_factor(jc.CORR3)
    want, want_u, want_z, _ = _ok(hip, group, F, 257, first=first, streams=[7, 0, 1023], flags=SOBOL)
    x, u, z = sd.joint_samples(distrs, 257, SEED, corr=jc.CORR3, streams=[7, 0, 1023], first=first, qmc=True, return_uniforms=True,
                               return_normals=True)
    assert _same(x, want) and _same(u, want_u) and _same(z, want_z)
    xd = sd.joint_samples(distrs, 257, SEED, factor=F, streams=[7, 0, 1023], first=first, qmc=True, device=True)
    assert xd.is_cuda and _same(xd.cpu().numpy(), want)
    x1 = sd.quantiles([distrs[1]], [np.array([0.2, 0.5, 0.93])])[0]
    w, fc, info = sd.conditional_factor(jc.CORR3, [1])
    z_obs = sd.normal_scores([distrs[1]], x1[None, :])
    mu = np.ascontiguousarray((w @ z_obs).T)
    want, want_u, _, _ = _cok(hip, [group[0], group[2]], fc, 257, B=3, shift=mu, first=first, flags=SOBOL)
    x, u = sd.conditional_samples(distrs, 257, SEED, {1: x1}, corr=jc.CORR3, first=first, qmc=True, return_uniforms=True)
    assert x.shape == (3, 3, 257) and _same(x[:, [0, 2]], want) and _same(u[:, [0, 2]], want_u)
    assert np.array_equal(x[:, 1], np.tile(x1[:, None], (1, 257)))
    with pytest.raises(hip.MlmcHipError, match="stream 1024"):
        sd.samples(distrs, 4, SEED, streams=[0, 1, 1024], qmc=True)


def test_estimate_entries(hip):
    """Estimate.sample_components / sample_joint / sample_conditional with qmc=True are the tool's entries with qmc=True"""
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.tool import simple_distribution as sd
    dev, spec, M = _small_vector_storage()
    qe.device_cache_clear()
    q = make_root_quantity(dev, spec)['q']
    doms = Estimate.estimate_domains(q, dev)
    fns = [Legendre(7, tuple(doms[m])) for m in range(M)]
    est = Estimate(q, dev, fns[0])
    pdfs = est.construct_densities(tol=1e-8, orth_moments_tol=1e-4, moments_fns=fns)
    distrs = [d[0] for d in pdfs]
    n, first = 256, 1024
    draws, ok = est.sample_components(n, SEED, densities=pdfs, first=first, qmc=True)
    assert draws.shape == (M, n) and ok.shape == (M,)
    for m in range(M):
        assert _same(draws[m], distrs[m].rvs(n, SEED, stream=m, first=first, qmc=True)), m
    assert not _same(draws, est.sample_components(n, SEED, densities=pdfs, first=first)[0])
    corr = np.array([[1.0, 0.5, 0.2, 0.0], [0.5, 1.0, 0.3, 0.1], [0.2, 0.3, 1.0, -0.4], [0.0, 0.1, -0.4, 1.0]])
    F, _ = sd.correlation_factor(corr)
    joint, _, used = est.sample_joint(n, SEED, corr=corr, densities=pdfs, first=first, qmc=True)
    assert _same(joint, sd.joint_samples(distrs, n, SEED, factor=F, first=first, qmc=True)) and np.array_equal(used, F @ F.T)
    assert not _same(joint, est.sample_joint(n, SEED, corr=corr, densities=pdfs, first=first)[0])
    given = {1: float(sd.quantiles([distrs[1]], [np.array([0.3])])[0][0])}
    cond, _, info = est.sample_conditional(n, SEED, given, corr=corr, densities=pdfs, first=first, qmc=True)
    assert _same(cond, sd.conditional_samples(distrs, n, SEED, given, corr=corr, first=first, qmc=True))
    assert not _same(cond, est.sample_conditional(n, SEED, given, corr=corr, densities=pdfs, first=first)[0])
    on_dev, _, _ = est.sample_conditional(n, SEED, given, corr=corr, densities=pdfs, first=first, qmc=True, device=True)
    assert on_dev.is_cuda and _same(on_dev.cpu().numpy(), cond)
