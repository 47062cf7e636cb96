"""GPU tests of the batched, seeded sampling from the max-entropy densities (k_q_sample in mlmc_amd/csrc/density.hip) through the
public entries: simple_distribution.samples, SimpleDistribution / Distribution .rvs, Estimate.sample_components and
mlmc_density_sample_batch.

A draw is x_j = Q(u_j) (include/mlmc_hip.h).  The uniforms are compared bit for bit with their NumPy restatement
(tests/sample_cases.py), the draws bit for bit with mlmc_density_quantiles_batch at those uniforms, and, independently of the
device's quantile route, with the long-double Fhat of tests/quantile_cases.py under the tolerance of the quantile checks."""
import ctypes as C

import numpy as np
import pytest

from tests import maxent_cases as mc
from tests import quantile_cases as qc
from tests import sample_cases as sc
from tests.test_gpu_quantiles import _dist, _fn, _raw_args

pytestmark = pytest.mark.gpu
# mixture and shifted Legendre, and one case each of the Fourier, spline, transformed and log = True kinds of the table
CASES = ("mix_R9", "shifted_R6", "fourier_R9", "spline_R10", "norm12_R21", "log_legendre_R8")
N_CYCLE = (0, 1, 2, 255, 256, 257, 1000)             # workgroup edges and an empty problem
SEED = 0x9E3779B97F4A7C15
FAR = 2 ** 33 + 1                                    # the high counter word and an odd start


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


@pytest.fixture(scope="module")
def table(hip):
    """per rule of qc.RULES the six cases at the multipliers the device solver returns at tol = 1e-8, with their long-double
    tables; problem k of rule r has n = N_CYCLE[(k + 6 r) % 7] draws, so the two batches cover every size"""
    from mlmc_amd.tool import simple_distribution as sd
    out = []
    for r, quad in enumerate(qc.RULES):
        group = []
        for k, name in enumerate(CASES):
            case = mc.cases()[name]
            lam, _, _, info = sd._solve_on_device(_fn(case), case.mu, case.sigma, case.domain, case.lam0, 1e-8, 100,
                                                  n_intervals=quad[0], gauss_degree=quad[1])
            assert info.success == 1, (name, quad)
            group.append(dict(case=case, lam=lam, quad=quad, ref=qc.RuleTable(case, lam, quad), dist=_dist(case, lam, quad),
                              n=N_CYCLE[(k + 6 * r) % len(N_CYCLE)], tag=f"{name} {quad[0]}x{quad[1]}"))
        out.append(group)
    assert {p["n"] for g in out for p in g} == set(N_CYCLE)
    return out


def _call(hip, group, quad, n, seed, streams=None, first=None, flags=0, kind=None, want_u=True, want_mass=False):
    """mlmc_density_sample_batch on the problems of `group`; returns (rc, out, u, mass) with out / u as NumPy arrays"""
    import torch
    kind = hip.HOST if kind is None else kind
    B = len(group)
    handles, r1, lam, sig = _raw_args(hip, group)
    a = np.array([p["case"].domain[0] for p in group], dtype=np.float64)
    b = np.array([p["case"].domain[1] for p in group], dtype=np.float64)
    n = np.ascontiguousarray(n, dtype=np.int64)
    total = int(np.sum(np.maximum(n, 0)))
    st = None if streams is None else np.ascontiguousarray(streams, dtype=np.uint32)
    fi = None if first is None else np.ascontiguousarray(first, dtype=np.int64)
    if kind == hip.DEVICE:
        out = torch.full((total,), 7.25, dtype=torch.float64, device="cuda")
        u = torch.full((total,), 7.25, dtype=torch.float64, device="cuda") if want_u else None
        torch.cuda.synchronize()
    else:
        out = np.full(total, 7.25)
        u = np.full(total, 7.25) if want_u else None
    mass = np.full(B, -1.0) if want_mass else None
    rc = hip.lib().mlmc_density_sample_batch(B, C.cast(handles, C.c_void_p), hip.ptr(r1), hip.ptr(lam), hip.ptr(sig), hip.ptr(a),
                                             hip.ptr(b), quad[0], quad[1], seed, hip.ptr(st), hip.ptr(fi), hip.ptr(n), flags,
                                             hip.ptr(out), hip.ptr(u), hip.ptr(mass), kind)
    if kind == hip.DEVICE:
        out, u = out.cpu().numpy(), None if u is None else u.cpu().numpy()
    return rc, out, u, mass


def _quantiles_c(hip, group, quad, p, n):
    """mlmc_density_quantiles_batch at the probabilities p (the problems' one after another, counts n)"""
    handles, r1, lam, sig = _raw_args(hip, group)
    a = np.array([pr["case"].domain[0] for pr in group], dtype=np.float64)
    b = np.array([pr["case"].domain[1] for pr in group], dtype=np.float64)
    n = np.ascontiguousarray(n, dtype=np.int64)
    p = np.ascontiguousarray(p, dtype=np.float64)
    out, mass = np.full(p.shape, 7.25), np.full(len(group), -1.0)
    hip.check(hip.lib().mlmc_density_quantiles_batch(len(group), C.cast(handles, C.c_void_p), hip.ptr(r1), hip.ptr(lam), hip.ptr(sig),
                                                     hip.ptr(a), hip.ptr(b), quad[0], quad[1], hip.ptr(p), hip.ptr(n), hip.ptr(out),
                                                     hip.ptr(mass), hip.HOST))
    return out, mass


def _want_uniforms(seed, streams, first, n, antithetic=False):
    return np.concatenate([sc.uniforms(seed, s, f, k, antithetic) for s, f, k in zip(streams, first, n)] + [np.zeros(0)])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def test_uniforms_and_inversion(hip, table):
    """u_out == the NumPy uniforms and out == mlmc_density_quantiles_batch(u_out), bit for bit, for host and device arrays, default
    and explicit streams, first = 0 and first = 2^33 + 1, without u_out, and with the masses of the quantile entry"""
    for group in table:
        quad, B = group[0]["quad"], len(group)
        n = [p["n"] for p in group]
        streams = [5, 0, 2 ** 32 - 1, 11, 11, 7]
        for st, first in ((None, None), (streams, [0, 3, FAR, 1, 1, 2 ** 62])):
            rc, out, u, mass = _call(hip, group, quad, n, SEED, st, first, want_mass=True)
            hip.check(rc)
            want_u = _want_uniforms(SEED, range(B) if st is None else st, [0] * B if first is None else first, n)
            assert _same(u, want_u), (quad, st)
            want, want_mass = _quantiles_c(hip, group, quad, u, n)
            assert _same(out, want) and np.array_equal(mass, want_mass), (quad, st)
            assert np.all(np.isfinite(out))
            rc, out_d, u_d, _ = _call(hip, group, quad, n, SEED, st, first, kind=hip.DEVICE)
            hip.check(rc)
            assert _same(u_d, want_u) and _same(out_d, want), (quad, st)
            for kind in (hip.HOST, hip.DEVICE):
                rc, out_n, u_n, _ = _call(hip, group, quad, n, SEED, st, first, kind=kind, want_u=False)
                hip.check(rc)
                assert u_n is None and _same(out_n, want), (quad, st, kind)


def test_python_entries(hip, table):
    """samples / rvs / quantiles agree bit for bit with each other and with the NumPy uniforms; device tensors hold the same bits"""
    import torch
    from mlmc_amd.tool import simple_distribution as sd
    from mlmc_amd.tool.distribution import Distribution
    for group in table:
        distrs = [p["dist"] for p in group]
        n = [p["n"] for p in group]
        xs, us = sd.samples(distrs, n, SEED, return_uniforms=True)
        assert len(xs) == len(us) == len(group)
        want = sd.quantiles(distrs, us)
        for k, (p, x, u, w) in enumerate(zip(group, xs, us, want)):
            assert x.shape == (p["n"],) and _same(u, sc.uniforms(SEED, k, 0, p["n"])) and _same(x, w), p["tag"]
            assert _same(p["dist"].rvs(p["n"], SEED, stream=k), x), p["tag"]
            assert _same(p["dist"].quantile(u), x), p["tag"]
        dev, dev_u = sd.samples(distrs, n, SEED, device=True, return_uniforms=True)
        for x, u, d, du in zip(xs, us, dev, dev_u):
            assert isinstance(d, torch.Tensor) and d.is_cuda and d.dtype == torch.float64
            assert _same(d.cpu().numpy(), x) and _same(du.cpu().numpy(), u)
        assert all(_same(a, b) for a, b in zip(sd.samples(distrs, n, SEED), xs))
        # one n / first for all, explicit streams
        xs2 = sd.samples(distrs, 257, SEED, streams=[3] * len(group), first=FAR, antithetic=True)
        u2 = sc.uniforms(SEED, 3, FAR, 257, True)
        for p, x, w in zip(group, xs2, sd.quantiles(distrs, u2)):
            assert _same(x, w) and _same(p["dist"].rvs(257, SEED, stream=3, first=FAR, antithetic=True), x), p["tag"]
    pr = table[0][0]
    old = _dist(pr["case"], pr["lam"], pr["quad"], Distribution)
    assert _same(old.rvs(1000, 7, stream=2, first=5), pr["dist"].rvs(1000, 7, stream=2, first=5))
    got = pr["dist"].rvs(300, 7, device=True)
    assert got.is_cuda and _same(got.cpu().numpy(), pr["dist"].rvs(300, 7))
    assert sd.samples([], 10, SEED) == []


def test_independence(hip, table):
    """a problem alone == anywhere in a batch; first = 50, n = 100 == [50:150] of n = 150; two calls give the same bits"""
    rng = np.random.default_rng(3)
    for group in table:
        quad, B = group[0]["quad"], len(group)
        streams = np.arange(10, 10 + B)
        rc, whole, whole_u, _ = _call(hip, group, quad, [150] * B, SEED, streams)
        hip.check(rc)
        rc, again, again_u, _ = _call(hip, group, quad, [150] * B, SEED, streams)
        assert rc == 0 and _same(again, whole) and _same(again_u, whole_u)
        rc, part, part_u, _ = _call(hip, group, quad, [100] * B, SEED, streams, [50] * B)
        hip.check(rc)
        whole, whole_u = whole.reshape(B, 150), whole_u.reshape(B, 150)
        assert _same(part.reshape(B, 100), whole[:, 50:]) and _same(part_u.reshape(B, 100), whole_u[:, 50:])
        perm = rng.permutation(B)
        rc, shuffled, _, _ = _call(hip, [group[i] for i in perm], quad, [150] * B, SEED, streams[perm])
        hip.check(rc)
        assert _same(shuffled.reshape(B, 150), whole[perm])
        for k in (0, B - 1):
            rc, alone, _, _ = _call(hip, [group[k]], quad, [150], SEED, [streams[k]])
            assert rc == 0 and _same(alone, whole[k]), group[k]["tag"]
        # other launch geometries of the same draws: 1500 copies of a problem (more workgroups than CUs), and a problem with
        # 70000 draws beside small ones (several workgroups in y)
        rc, copies, _, _ = _call(hip, [group[0]] * 1500, quad, [150] * 1500, SEED, [streams[0]] * 1500, want_u=False)
        assert rc == 0 and _same(copies.reshape(1500, 150), np.tile(whole[0], (1500, 1)))
        rc, big, _, _ = _call(hip, group[:3], quad, [2, 70000, 150], SEED, streams[:3], want_u=False)
        assert rc == 0 and _same(big[:2], whole[0, :2]) and _same(big[2:152], whole[1]) and _same(big[70002:], whole[2])


def test_antithetic(hip, table):
    """u[2k + 1] == 1 - u[2k], the uniforms are the restatement's, and out is the quantiles of exactly those"""
    for group in table:
        quad, B = group[0]["quad"], len(group)
        for first in (0, FAR):
            n = [p["n"] for p in group]
            rc, out, u, _ = _call(hip, group, quad, n, SEED, None, [first] * B, flags=1)
            hip.check(rc)
            assert _same(u, _want_uniforms(SEED, range(B), [first] * B, n, True))
            assert _same(out, _quantiles_c(hip, group, quad, u, n)[0])
        rc, out, u, _ = _call(hip, group, quad, [1000] * B, SEED, flags=1)
        hip.check(rc)
        u, out = u.reshape(B, 1000), out.reshape(B, 1000)
        assert np.array_equal(u[:, 1::2], 1.0 - u[:, ::2])
        assert np.array_equal(u[:, ::2], np.array([sc.uniforms(SEED, s, 0, 500) for s in range(B)]))
        assert _same(out.reshape(-1), _quantiles_c(hip, group, quad, u.reshape(-1), [1000] * B)[0])


def test_against_the_long_double_reference(hip, table):
    """n = 1000 draws of every problem: |Fhat_ref(x_j) - u_j| in the units and under the tolerance of the quantile checks
    (qc.quantile_units, qc.quantile_tolerance); independent of the device's quantile route"""
    failures = []
    print()
    for group in table:
        quad, B = group[0]["quad"], len(group)
        rc, out, u, _ = _call(hip, group, quad, [1000] * B, 7)
        hip.check(rc)
        want_u = _want_uniforms(7, range(B), [0] * B, [1000] * B)
        assert _same(u, want_u)
        for pr, x, p in zip(group, out.reshape(B, 1000), want_u.reshape(B, 1000)):
            a, b = pr["case"].domain
            assert np.all((x >= a) & (x <= b)), pr["tag"]
            units = qc.quantile_units(pr["ref"], p, x)
            k = int(np.argmax(units))
            tol = qc.quantile_tolerance(pr["case"])
            print(f"{pr['tag']:28s} worst {units[k]:8.4g} units at u = {p[k]:.6g} (tolerance {tol:g})")
            if not units[k] <= tol:
                failures.append(f"{pr['tag']}: {units[k]:.4g} units at u = {p[k]:.6g} (tolerance {tol:g})")
    assert not failures, "\n".join(failures)


def test_kolmogorov_distance_on_the_device(hip, table):
    """16384 draws of mix_R9 under seed 7, streams 0 and 11: their Kolmogorov distance from the long-double Fhat is at most the
    DKW bound at confidence 1 - 1e-9, 0.02557, + 1e-9 for the error of the inversion"""
    pr = [p for p in table[0] if p["case"].name == "mix_R9"][0]
    print()
    for stream in (0, 11):
        x = pr["dist"].rvs(sc.DKW_N, 7, stream=stream)
        F, _ = pr["ref"].fhat(x)
        d = sc.kolmogorov_distance(F)
        print(f"mix_R9 seed 7 stream {stream}: Kolmogorov distance {d:.4f} (bound {sc.DKW_BOUND:.5f})")
        assert d <= sc.DKW_BOUND + 1e-9, (stream, d)


def test_row_beyond_the_lds_cap(hip, table):
    """n_intervals = 20000: the P row (160 KB) does not fit in the LDS the kernel asks for and is read from global memory;
    the draws still equal the quantile entry's bit for bit"""
    from mlmc_amd.tool import simple_distribution as sd
    pr = [p for p in table[0] if p["case"].name == "mix_R9"][0]
    d = _dist(pr["case"], pr["lam"], (20000, 21))
    x, u = sd.samples([d, d], [257, 3], SEED, streams=[4, 9], return_uniforms=True)
    assert _same(u[0], sc.uniforms(SEED, 4, 0, 257)) and _same(u[1], sc.uniforms(SEED, 9, 0, 3))
    want = sd.quantiles([d, d], u)
    assert _same(x[0], want[0]) and _same(x[1], want[1]) and np.all(np.isfinite(x[0]))
    a, b = pr["case"].domain
    assert np.all((x[0] > a) & (x[0] < b)) and len(np.unique(x[0])) == 257


def test_long_lists(hip, table):
    """4 200 001 draws of one problem, and 2 x 2 100 000 of two: every lane walks a list of about 16 draws and starts each one
    while its neighbours are in the middle of theirs; the draws still equal the quantile entry's at the same uniforms bit for
    bit (compared on the device), and the first 1000 are the draws of a call of 1000"""
    import torch
    from mlmc_amd.tool import simple_distribution as sd
    mix = [p for p in table[0] if p["case"].name == "mix_R9"][0]
    spl = [p for p in table[0] if p["case"].name == "spline_R10"][0]
    for distrs, n, streams in (([mix["dist"]], 4_200_001, [6]), ([spl["dist"], mix["dist"]], 2_100_000, [6, 6])):
        x, u = sd.samples(distrs, n, SEED, streams=streams, device=True, return_uniforms=True)
        want = sd.quantiles(distrs, u)
        for xb, ub, wb, d in zip(x, u, want, distrs):
            assert xb.shape == (n,) and torch.equal(xb, wb) and bool(torch.isfinite(xb).all())
            assert _same(ub[:1000].cpu().numpy(), sc.uniforms(SEED, 6, 0, 1000)) and _same(ub[-3:].cpu().numpy(), sc.uniforms(SEED, 6, n - 3, 3))
            assert _same(xb[:1000].cpu().numpy(), d.rvs(1000, SEED, stream=6))


def test_more_coefficients_than_the_lds_holds(hip):
    """a transformed basis over 601 Fourier terms: 601 effective coefficients, more than the 512 the kernel stages, so coefficients
    and row are read from global memory; the draws equal the quantile entry's bit for bit"""
    import mlmc_amd
    from mlmc_amd.tool import simple_distribution as sd
    dom = (-4.0, 6.0)
    size, K = 601, 5
    matrix = np.zeros((K, size))
    matrix[np.arange(K), np.arange(K)] = 1.0
    matrix[1, 600] = 0.125                               # the last coefficient is in use
    fn = mlmc_amd.TransformedMoments(mlmc_amd.Fourier(size, dom), matrix)
    d = sd.SimpleDistribution(fn, np.stack([np.eye(K)[0], np.ones(K)], axis=1), domain=dom)
    d.multipliers, d._moment_errs = np.array([np.log(10.0), 0.7, -0.4, 0.2, 0.1]), np.ones(K)
    for n in (257, 70000):
        x, u = sd.samples([d, d], [n, 3], SEED, streams=[1, 2], return_uniforms=True)
        assert _same(u[0], sc.uniforms(SEED, 1, 0, n)) and _same(u[1], sc.uniforms(SEED, 2, 0, 3))
        want = sd.quantiles([d, d], u)
        assert _same(x[0], want[0]) and _same(x[1], want[1])
        assert np.all((x[0] > dom[0]) & (x[0] < dom[1]))


def test_degenerate_problems(hip, table):
    """NaN multipliers, and a domain that reaches outside the domain of the moments (the mass is NaN): NaN draws, u_out intact, no
    error; the other problems of the batch are unchanged"""
    group = list(table[0][:4])
    quad = group[0]["quad"]
    bad = dict(group[1])
    bad["lam"] = np.full_like(group[1]["lam"], np.nan)
    one_nan = dict(group[3])
    one_nan["lam"] = group[3]["lam"].copy()
    one_nan["lam"][-1] = np.nan
    n = [300, 257, 150, 2]
    rc, want, want_u, want_mass = _call(hip, group, quad, n, SEED, want_mass=True)
    hip.check(rc)
    for kind in (hip.HOST, hip.DEVICE):
        rc, out, u, mass = _call(hip, [group[0], bad, group[2], one_nan], quad, n, SEED, kind=kind, want_mass=True)
        hip.check(rc)
        assert _same(u, want_u) and _same(u, _want_uniforms(SEED, range(4), [0] * 4, n))
        assert np.all(np.isnan(out[300:557])) and np.all(np.isnan(out[707:]))
        assert _same(out[:300], want[:300]) and _same(out[557:707], want[557:707]) and mass[0] == want_mass[0] and mass[2] == want_mass[2]
    from mlmc_amd.tool import simple_distribution as sd
    pr = group[0]
    wide = _dist(pr["case"], pr["lam"], quad)
    wide.domain = (pr["case"].domain[0] - 1.0, pr["case"].domain[1])
    x, u = sd.samples([pr["dist"], wide, pr["dist"]], 300, SEED, streams=[0, 1, 0], return_uniforms=True)
    assert np.all(np.isnan(x[1])) and _same(u[1], sc.uniforms(SEED, 1, 0, 300))
    assert _same(x[0], want[:300]) and _same(x[2], want[:300])


def test_errors_and_no_ops(hip, table):
    group = list(table[0][:4])
    quad = group[0]["quad"]
    name = "mlmc_density_sample_batch"
    n = [2, 2, 2, 2]

    def expect(rc, pattern):
        with pytest.raises(hip.MlmcHipError, match=pattern):
            hip.check(rc)
    assert _call(hip, group, quad, n, 1)[0] == 0
    expect(_call(hip, group, quad, [2, -1, 2, 2], 1)[0], name + ": problem 1.*n < 0")
    expect(_call(hip, group, quad, n, 1, first=[0, 0, -1, 0])[0], name + ": problem 2.*first < 0")
    expect(_call(hip, group, quad, n, 1, first=[0, 0, 0, 2 ** 63 - 2])[0], name + ": problem 3.*overflow")
    assert _call(hip, group, quad, n, 1, first=[0, 0, 0, 2 ** 63 - 3])[0] == 0
    expect(_call(hip, group, quad, n, 1, kind=5)[0], name + ": bad mem_kind")
    expect(_call(hip, group, quad, n, 1, flags=2)[0], name + ": unknown flag")
    expect(_call(hip, group, quad, n, 1, flags=-1)[0], name + ": unknown flag")
    for pattern in ("bad mem_kind", "unknown flag"):
        with pytest.raises(hip.MlmcHipError) as err:
            hip.check(_call(hip, group, quad, n, 1, kind=5 if pattern == "bad mem_kind" else hip.HOST, flags=0 if pattern == "bad mem_kind" else 4)[0])
        assert "problem" not in str(err.value)
    # a null basis and a >= b name the problem
    handles, r1, lam, sig = _raw_args(hip, group)
    B = len(group)
    a = np.array([p["case"].domain[0] for p in group])
    b = np.array([p["case"].domain[1] for p in group])
    nn = np.array(n, dtype=np.int64)
    out, u = np.full(8, 7.25), np.full(8, 7.25)
    P = hip.ptr
    lib = hip.lib()

    def raw(h=handles, a=a, b=b, B=B, n=nn, out=out):
        return lib.mlmc_density_sample_batch(B, C.cast(h, C.c_void_p), P(r1), P(lam), P(sig), P(a), P(b), quad[0], quad[1], 1, None, None,
                                             P(n), 0, P(out), P(u), None, hip.HOST)
    assert raw() == 0
    null_h = (C.c_void_p * B)(*[_fn(p["case"])._basis_handle().value for p in group])
    null_h[2] = None
    expect(raw(h=null_h), name + ": problem 2.*null basis")
    bad_b = b.copy()
    bad_b[3] = a[3]
    expect(raw(b=bad_b), name + ": problem 3.*domain")
    expect(raw(B=-1), name + ".*B < 0")
    expect(raw(out=None), name + ".*null")
    # no-ops: B = 0, and no draws at all (the arrays may be NULL then and are not touched)
    assert lib.mlmc_density_sample_batch(0, None, None, None, None, None, None, 0, 0, 1, None, None, None, 0, None, None, None, hip.HOST) == 0
    out[:] = 7.25
    assert raw(n=np.zeros(B, dtype=np.int64)) == 0 and np.all(out == 7.25)
    assert raw(n=np.zeros(B, dtype=np.int64), out=None) == 0
    rc, _, _, mass = _call(hip, group, quad, [0] * B, 1, want_mass=True)
    assert rc == 0 and np.array_equal(mass, _quantiles_c(hip, group, quad, np.zeros(0), [0] * B)[1]) and np.all(mass > 0)


def test_kernel_time_counts_the_sampling_kernel(hip, table):
    group = table[0]
    ms, launches = C.c_double(), C.c_int64()
    hip.check(hip.lib().mlmc_density_quantiles_kernel_time(C.byref(ms), C.byref(launches)))
    hip.check(_call(hip, group, group[0]["quad"], [1000] * len(group), 1)[0])
    hip.check(hip.lib().mlmc_density_quantiles_kernel_time(C.byref(ms), C.byref(launches)))
    assert launches.value == 1 and ms.value > 0


# ---- Estimate.sample_components -------------------------------------------------------------------------------------------
def _small_vector_storage():
    import torch
    from tests.util import level_arrays
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    from mlmc_amd.sample_storage import DeviceMemory
    M, steps = 4, [0.5, 0.07, 0.01]
    levels = level_arrays([2000, 2000, 2000], steps, M, 0, seed=78)
    spec = [QuantitySpec(name="q", unit="m", shape=(4, 1), times=[1], locations=['0'])]
    dev = DeviceMemory()
    dev.save_global_data(result_format=spec, level_parameters=[[s] for s in steps])
    for l, (f, c) in enumerate(levels):
        f = f.copy()
        c = np.zeros_like(f) if c is None else c.copy()
        for m in range(M):
            for arr in (f, c):
                arr[m] = 0.1 * (m - 2) + (0.7 + 0.05 * m) * (arr[m] - 0.125 * m)
        f[1, 7::53] = np.nan
        dev.set_level_samples(l, torch.from_numpy(np.stack([f, c], axis=-1)).cuda())
    return dev, spec, M


def test_estimate_sample_components(hip):
    import torch
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.quantity.quantity import make_root_quantity
    dev, spec, M = _small_vector_storage()
    qe.device_cache_clear()
    q = make_root_quantity(dev, spec)['q']
    doms = Estimate.estimate_domains(q, dev)
    fns = [Legendre(7, tuple(doms[m])) for m in range(M)]
    est = Estimate(q, dev, fns[0])
    n = 1000
    draws, ok = est.sample_components(n, SEED, tol=1e-8, orth_moments_tol=1e-4, moments_fns=fns)
    assert draws.shape == (M, n) and draws.dtype == np.float64 and ok.shape == (M,) and ok.dtype == bool
    pdfs = est.construct_densities(tol=1e-8, orth_moments_tol=1e-4, moments_fns=fns)
    for m in range(M):
        assert _same(draws[m], pdfs[m][0].rvs(n, SEED, stream=m)), m
        assert np.all((draws[m] >= doms[m][0]) & (draws[m] <= doms[m][1]))
    _, ok_q = est.estimate_component_quantiles([0.5], tol=1e-8, orth_moments_tol=1e-4, moments_fns=fns)
    assert np.array_equal(ok, ok_q) and np.array_equal(ok, np.array([bool(d[2].success) for d in pdfs]))
    again, ok2 = est.sample_components(n, SEED, densities=pdfs)
    assert _same(again, draws) and np.array_equal(ok2, ok)
    on_dev, ok3 = est.sample_components(n, SEED, densities=pdfs, device=True)
    assert isinstance(on_dev, torch.Tensor) and on_dev.is_cuda and on_dev.shape == (M, n) and on_dev.dtype == torch.float64
    assert _same(on_dev.cpu().numpy(), draws) and np.array_equal(ok3, ok)
    cont, _ = est.sample_components(100, SEED, densities=pdfs, first=900, antithetic=True)
    for m in range(M):
        assert _same(cont[m], pdfs[m][0].rvs(100, SEED, stream=m, first=900, antithetic=True))
