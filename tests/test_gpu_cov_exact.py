"""GPU checks of the covariance kernels (k_cov_accum<T = 1, 2, 4>, k_cov_accum_t4<MODE 0 / 2 / 3>, k_cov_accum_t4_rows, the
64 x 64 blocks of 65..128 moments, the values route with k_apply_matrix_mfma and the difference Gram, k_cov_lin_mean with its inner
accumulators, k_spline_band_accum) through engine.LevelAccumulator against the 80-bit long-double reference of
tests/cov_exact.py, in units of 2^-53 * scale.  Cases, routes and tolerances are those of tests/cov_cases.py: the tolerance of a
class is max(16, 4 x the worse fp64 twin), calibrated without a device by tests/test_cov_exact_cpu.py.  No entry, level or case is
left out; a zero scale demands an exact zero; a non-finite value fails except sp = NaN of a mean-only accumulator.  Every route
is asserted to have run: launch counts of the matrix and auxiliary passes and the executed matrix-core flops (26 against 42
tiles per pair at 33..64 moments).  Every test prints its worst units with the place (pytest -s)."""
import numpy as np
import pytest

from tests import accum_exact as ax
from tests import cov_cases as cc
from tests.test_gpu_gram_exact import Worst

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    assert _lib.device_info()["n_cu"] <= cc.N_CU           # the long levels exceed a full grid
    return _lib


def _fn(case):
    from mlmc_amd import Fourier, Legendre, Monomial, Spline, TransformedMoments
    d = case.desc
    cls = {ax.LEGENDRE: Legendre, ax.MONOMIAL: Monomial, ax.FOURIER: Fourier, ax.SPLINE: Spline}[d.kind]
    fn = cls(d.size, d.domain, log=d.log, safe_eval=d.safe_eval)
    assert fn._linear_scale == d.scale and fn._linear_shift == d.shift and tuple(fn.ref_domain) == d.ref_domain
    return fn if case.matrix is None else TransformedMoments(fn, case.matrix)


def _set_route(monkeypatch, env):
    """the switches are read when an accumulator is created"""
    for key in cc.ALL_ENV:
        monkeypatch.delenv(key, raising=False)
    for key, value in env.items():
        monkeypatch.setenv(key, value)


def _run(case, chunks, device=False, mean_only=False):
    """chunks: [(level, fine [M, n], coarse [M, n] | None)] -> (n, n_rm, s, sp), (matrix launches, auxiliary launches, flops)"""
    import torch
    from mlmc_amd.engine import LevelAccumulator
    mode = LevelAccumulator.MOMENTS if case.entry == "diff" else LevelAccumulator.COV
    acc = LevelAccumulator(_fn(case), case.L, mode, n_comp=case.M, mean_only=mean_only)
    acc.kernel_time()
    acc.aux_kernel_time()
    acc.kernel_flops()
    for l, f, c in chunks:
        fa = np.ascontiguousarray(f if case.M > 1 else f[0])
        ca = None if c is None else np.ascontiguousarray(c if case.M > 1 else c[0])
        if device:
            fa = torch.from_numpy(fa).cuda()
            ca = None if ca is None else torch.from_numpy(ca).cuda()
        acc.push(l, fa, ca)
    out = acc.finalize()
    ran = (acc.kernel_time()[1], acc.aux_kernel_time()[1], acc.kernel_flops())
    acc.close()
    return out, ran


def _whole(case):
    return [(l, f, c) for l, (f, c) in enumerate(case.levels)]


def _tiles(kernel, pair, mode):
    """16 x 16 output tiles per sample of the diagonal-block kernels (cov.hip, cov_tiles_per_sample); mode 0: three Gram
    matrices, 3: the two of the variance, 2: G0 only"""
    T = {"t1": 1, "t2": 2, "t4": 4}[kernel]
    full, upper = T * T, T * (T + 1) // 2
    if mode == 0:
        return 2 * full + upper if pair else 2 * upper
    if mode == 3:
        return full + upper if pair else upper
    return full if pair else upper


def _expected_flops(case, chunks, route, lin_min_n=0):
    """matrix-core flops of a scalar covariance of at most 64 plain moments under a route"""
    lin = route.startswith("lin") and cc.lin_eligible(case.desc, case.matrix)
    total = 0
    for l, f, c in chunks:
        n = f.shape[1]
        on_lin = lin and n >= lin_min_n
        if on_lin and c is None and cc.lin0(case, route):
            continue                                                    # no matrix pass at all
        total += 512 * _tiles(case.kernel, c is not None, 3 if on_lin else 0) * n
    return total


def _assert_route(case, chunks, route, ran, lin_min_n=0):
    launches, aux, flops = ran
    lin = route.startswith("lin") and cc.lin_eligible(case.desc, case.matrix)
    assert (aux > 0) == lin, (case, route, ran)
    if case.entry == "diff":
        return                                                          # the difference Gram rides along with the moments kernel
    assert launches > 0 and flops > 0, (case, route, ran)
    assert _tiles("t4", True, 3) == 26 and _tiles("t4", True, 0) == 42
    if case.entry == "cov" and case.matrix is None and case.M == 1 and case.desc.size <= 128:
        # one matrix launch per 64 x 64 block of every chunk: all NB^2 blocks of a pair chunk, the upper NB (NB + 1) / 2 without
        # coarse values (the reduction mirrors them); none for a chunk whose second moments are linearised too
        NB = (case.desc.size + 63) // 64
        want = sum(NB * NB if c is not None else NB * (NB + 1) // 2 for _, f, c in chunks
                   if not (lin and c is None and f.shape[1] >= lin_min_n and cc.lin0(case, route)))
        assert launches == want, (case, route, launches, want)
    if case.entry == "cov" and case.matrix is None and case.M == 1 and case.desc.size <= 64 and case.desc.kind != ax.SPLINE:
        assert flops == _expected_flops(case, chunks, route, lin_min_n), (case, route, flops, _expected_flops(case, chunks, route, lin_min_n))


def _judge(case, route, got, label, worst, mean_only=False):
    """counts exactly; every entry of s and sp in units against the reference; exact zeros where the scale is zero (unit_errors);
    bitwise symmetry; the P_0 P_0 entries; sp = NaN under mean_only"""
    ref = cc.reference(case)
    n, n_rm, s, sp = got
    assert np.array_equal(n, ref.n) and np.array_equal(n_rm, ref.n_rm), (case, label, n, ref.n, n_rm, ref.n_rm)
    assert s.shape == ref.s.shape and sp.shape == ref.sp.shape, (case, s.shape, ref.s.shape)
    Ro, M = case.Rout, case.M
    for l, (f, c) in enumerate(case.levels):
        if case.entry == "cov":
            for q, v in (("s", s[l]),) if mean_only and case.kernel != "vals" else (("s", s[l]), ("sp", sp[l])):
                m3 = v.reshape(M, Ro, Ro)
                worst.check(np.array_equal(m3, m3.transpose(0, 2, 1)), q + " is not bitwise symmetric", case, label, l)
            if case.matrix is None:
                want = 0.0 if c is not None else float(n[l])            # phi_0 = 1: the exact count, or an exact zero
                for q, v in (("s", s[l]), ("sp", sp[l])):
                    first = v.reshape(M, Ro * Ro)[:, 0]
                    if not np.all(np.isnan(first)):                     # (sp of a mean-only accumulator: judged below)
                        worst.check(bool(np.all(first == want)), "the P0 P0 entry of " + q, case, label, l, first.tolist(), want)
        quantities = ["s", "sp"]
        if mean_only and case.kernel != "vals":
            # (the values route has no pass that exists for sp alone: nothing is skipped, and its sp are held to the reference)
            worst.check(bool(np.all(np.isnan(sp[l]))), "sp of a mean-only accumulator is not NaN", case, label, l)
            quantities = ["s"]
        for q in quantities:
            key, want, scale = cc.judged(case, route, l, q)
            value = (s if q == "s" else sp)[l]
            units, flat = ax.worst(value, want, scale)
            per = Ro * Ro if case.entry == "cov" else Ro
            e = flat % per
            place = "{} [{}] level {} (n = {}) component {} entry {}".format(
                case.name, label, l, f.shape[1], flat // per, (e // Ro, e % Ro) if case.entry == "cov" else e)
            worst.add(" ".join(key), units, cc.tolerance(key), place)
            if key[1] == "lin":                                         # both units are reported; the linearised one is the gate
                other = "(in definitional units) " + " ".join(key)
                du = ax.worst(value, want, cc.judged(case, "direct", l, q)[2])[0]
                if other not in worst.w or du > worst.w[other][0]:
                    worst.w[other] = (du, float("inf"), place)


def _same_bits(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


GROUPS = {}
for _case in cc.cases().values():
    GROUPS.setdefault(_case.name.split("_")[0] + ("_" + _case.kernel if _case.name.startswith("legendre") else ""), []).append(_case)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_covariance_against_the_long_double_reference(hip, group, monkeypatch):
    """Every case of a group under each of its routes: host chunks against the reference, a second run bit-equal, device-resident
    chunks bit-equal to the host's, the intended route asserted; on the direct route also the mean-only accumulator (sp = NaN)
    and every level in ragged chunks from device tensors, each held to the reference on its own."""
    worst = Worst()
    for case in GROUPS[group]:
        whole = _whole(case)
        results = {}
        for route in case.routes:
            _set_route(monkeypatch, cc.ROUTES[route])
            got, ran = _run(case, whole)
            _assert_route(case, whole, route, ran)
            _judge(case, route, got, route, worst)
            again, ran2 = _run(case, whole)
            worst.check(_same_bits(got, again) and ran2 == ran, "a second run differs", case, route)
            dev, _ = _run(case, whole, device=True)
            worst.check(_same_bits(got, dev), "host and device-resident chunks differ", case, route)
            results[route] = (got, ran)
            if route == "lin" and not cc.lin_eligible(case.desc, case.matrix):      # safe_eval=False: stays direct, bit for bit
                worst.check(_same_bits(got, results["direct"][0]) and ran == results["direct"][1],
                            "an ineligible accumulator left the direct route", case)
            if route.startswith("lin") and cc.lin_eligible(case.desc, case.matrix):
                assert ran[2] < results["direct"][1][2], (case, route, ran, results["direct"][1])     # fewer Gram tiles
        # The switches that change no launch count did take effect: against "lin", the means of another family of extended sums
        # (CHEB=0) or of a full auxiliary pass instead of the matrix kernel's row sums (ROWSUMS=0, 49..64 moments) differ in some
        # bit, while the second moments of the pair levels -- the same matrix pass -- are bit-equal.
        pair = np.array([c is not None for _, c in case.levels])
        for route in ("lin_cheb0", "lin_rowsums0"):
            if route in results and cc.lin_eligible(case.desc, case.matrix):
                (_, _, s0, sp0), (_, _, s1, sp1) = results["lin"][0], results[route][0]
                worst.check(not np.array_equal(s0, s1), "the switch of this route changed nothing", case, route)
                worst.check(np.array_equal(sp0[pair], sp1[pair]), "the switch of this route changed the matrix pass", case, route)
        _set_route(monkeypatch, cc.ROUTES["direct"])
        if case.entry == "cov":
            mean, ran = _run(case, whole, mean_only=True)
            assert ran[1] == 0, (case, ran)
            _judge(case, "direct", mean, "mean_only", worst, mean_only=True)
        if not case.name.startswith("long_"):
            ragged = []
            for l, (f, c) in enumerate(case.levels):
                cuts = cc.ragged_cuts(f.shape[1])
                ragged += [(l, f[:, lo:hi], None if c is None else c[:, lo:hi]) for lo, hi in zip(cuts[:-1], cuts[1:])]
            got, ran = _run(case, ragged, device=True)
            _judge(case, "direct", got, "ragged", worst)
    worst.show(group)
    assert not worst.failures, worst.failures[:8]


@pytest.mark.parametrize("name", ["legendre_17", "legendre_64", "legendre_100", "monomial_33"])
def test_a_level_fed_from_both_sides_of_the_threshold(hip, name, monkeypatch):
    """MLMC_HIP_LINEARIZE_MIN_N = 100: the largest level with and the largest without coarse values in two chunks each, the first
    of 100 or more samples (linearised), the second shorter (three Gram matrices).  Each chunk is a level of its own in the
    reference; the unit of an entry is the sum of the units of its two chunks, the tolerance the larger of the two classes."""
    case = cc.cases()[name]
    Bp, B0 = cc.batches(case.kernel)
    picks = [[l for l, (f, c) in enumerate(case.levels) if f.shape[1] == n and (c is not None) == pair][0]
             for n, pair in ((4 * B0 + 3, False), (4 * Bp + 3, True))]
    levels, chunks = [], []
    for k, l in enumerate(picks):
        f, c = case.levels[l]
        cut = f.shape[1] - 31
        assert cut >= 100
        for lo, hi in ((0, cut), (cut, f.shape[1])):
            levels.append((f[:, lo:hi], None if c is None else c[:, lo:hi]))
            chunks.append((k, levels[-1][0], levels[-1][1]))
    split = cc.Case(name + "_split", case.desc, levels, case.kernel, ("lin",))
    ref = cc.reference(split)
    _set_route(monkeypatch, {"MLMC_HIP_LINEARIZE_MIN_N": "100"})
    two = cc.Case(name + "_two", case.desc, [case.levels[l] for l in picks], case.kernel, ("lin",))
    got, ran = _run(two, chunks)
    _assert_route(two, chunks, "lin", ran, lin_min_n=100)
    again, _ = _run(two, chunks, device=True)
    assert _same_bits(got, again), name
    n, n_rm, s, sp = got
    worst = Worst()
    for k in range(2):
        assert n[k] == ref.n[2 * k] + ref.n[2 * k + 1] and n_rm[k] == ref.n_rm[2 * k] + ref.n_rm[2 * k + 1]
        for q, value in (("s", s[k]), ("sp", sp[k])):
            (ka, wa, sa), (kb, wb, sb) = cc.judged(split, "lin", 2 * k, q), cc.judged(split, "direct", 2 * k + 1, q)
            units, flat = ax.worst(value, wa + wb, sa + sb)
            worst.add(" ".join(ka) + " + " + kb[1], units, max(cc.tolerance(ka), cc.tolerance(kb)),
                      "{} level {} entry ({}, {})".format(name, k, flat // case.Rout, flat % case.Rout))
    worst.show(name)
    assert not worst.failures, worst.failures
