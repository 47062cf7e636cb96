"""CPU checks of the extended-precision reference of the component covariance and of the bootstrap contraction
(tests/gram_exact.py): both functions against exact rational arithmetic on the same fp64 inputs, the conditions the case tables
of tests/gram_cases.py must satisfy without a device, the calibration of the fp64 twins (printed with pytest -s, pinned by
XCOV_TWIN_UNITS / BOOT_TWIN_UNITS, from which tests/test_gpu_gram_exact.py derives the device tolerances), and deliberately
broken twins that show what the gates catch."""
from fractions import Fraction

import numpy as np
import pytest

from tests import accum_exact as ax
from tests import gram_cases as gc
from tests import gram_exact as gx

LD = np.longdouble


def test_long_double_is_extended_precision():
    """without an 80-bit long double the module proves nothing: a failure, not a skip"""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


def _frac(v):
    """exact Fraction of a long double (or double)"""
    frac, exp = np.frexp(LD(v))
    hi = float(frac)
    return (Fraction(hi) + Fraction(float(frac - LD(hi)))) * Fraction(2) ** int(exp)


def _units(got, want, scale):
    """|got - want| / (2^-53 scale) in exact arithmetic; zero scale: 0 if both are zero"""
    err = abs(_frac(got) - want)
    if scale == 0:
        assert err == 0 and want == 0
        return 0.0
    return float(err / (scale * Fraction(1, 2 ** 53)))


# ---------------------------------------------------------------------------------------------------------------------------
# the reference against exact rational arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
def test_xcov_sums_against_fractions():
    """M = 3, n = 40, a level 0 and a pair level with NaNs and a shift: s, sp within 0.1 unit of the exact sums of the same fp64
    f~, c~; the scales to 2^-50"""
    rng = np.random.default_rng(1)
    M, n = 3, 40
    shift = np.array([0.3, -1.7, 1e3])
    f = rng.normal(size=(M, n)) * np.array([1.0, 1e-3, 50.0])[:, None] + shift[:, None]
    c = f + 0.01 * rng.normal(size=(M, n))
    f[1, 7] = np.nan
    c[2, 39] = np.nan
    levels = [(f.copy(), None), (f, c)]
    ref = gx.xcov_sums(levels, shift)
    assert list(ref.n) == [39, 38] and list(ref.n_rm) == [1, 2]
    worst = 0.0
    for l, (fl, cl) in enumerate(levels):
        keep, F, C = gx.xcov_kept(fl, cl, shift)
        for i in range(M):
            for j in range(M):
                s = sp = S = SP = Fraction(0)
                for k in range(F.shape[1]):
                    fi, fj = Fraction(float(F[i, k])), Fraction(float(F[j, k]))
                    ci, cj = (Fraction(0), Fraction(0)) if C is None else (Fraction(float(C[i, k])), Fraction(float(C[j, k])))
                    y = fi * fj - ci * cj
                    a = (abs(fi) + abs(ci)) * (abs(fj) + abs(cj))
                    s, sp, S, SP = s + y, sp + y * y, S + a, SP + a * a
                e = i * M + j
                worst = max(worst, _units(ref.s[l, e], s, S), _units(ref.sp[l, e], sp, SP))
                assert abs(_frac(ref.S[l, e]) - S) <= S * Fraction(1, 2 ** 50) and abs(_frac(ref.SP[l, e]) - SP) <= SP * Fraction(1, 2 ** 50)
    print("\nxcov_sums against Fraction: worst {:.3g} units".format(worst))
    assert worst <= 0.1


def _exact_legendre(t, R):
    p = [Fraction(1), t]
    for i in range(2, R):
        p.append(((2 * i - 1) * t * p[i - 1] - (i - 1) * p[i - 2]) / i)
    return p[:R]


def test_weighted_sums_against_fractions():
    """Legendre, R = 4, n = 40, a pair chunk with dropped samples, four replicates of multinomial weights: counts exactly, s, sp
    within 0.1 unit of the exact weighted sums of the rows at the same fp64 t; the scales to 2^-50"""
    rng = np.random.default_rng(2)
    R, n, nb = 4, 40, 4
    desc = ax.Desc(ax.LEGENDRE, R, (-3.0, 3.5))
    f = rng.normal(size=(1, n))
    c = f + 0.1 * rng.normal(size=(1, n))
    f[0, 3], c[0, 11], f[0, 20] = np.nan, 9.0, -3.5
    w = np.stack([rng.multinomial(s, np.full(n, 1.0 / n)) for s in (40, 23, 0, 31)])
    cnt, s, sp, S, SP = gx.weighted_sums(desc, f, c, w)
    tf, kf, _ = ax.transform(desc, f[0], np.float64)
    tc, kc, _ = ax.transform(desc, c[0], np.float64)
    keep = kf & kc
    assert keep.sum() == n - 3
    assert np.array_equal(cnt, (w * keep[None, :]).sum(axis=1)) and cnt[2] == 0
    worst = 0.0
    for b in range(nb):
        es, esp, eS, eSP = ([Fraction(0)] * R for _ in range(4))
        for i in np.flatnonzero(keep):
            pf, pc = _exact_legendre(Fraction(float(tf[i])), R), _exact_legendre(Fraction(float(tc[i])), R)
            wi = int(w[b, i])
            for r in range(R):
                d, a = pf[r] - pc[r], abs(pf[r]) + abs(pc[r])
                es[r] += wi * d
                esp[r] += wi * d * d
                eS[r] += wi * a
                eSP[r] += wi * (d * d + 2 * abs(d) * a)
        for r in range(R):
            worst = max(worst, _units(s[b, r], es[r], eS[r]), _units(sp[b, r], esp[r], eSP[r]))
            assert abs(_frac(S[b, r]) - eS[r]) <= eS[r] * Fraction(1, 2 ** 50) and abs(_frac(SP[b, r]) - eSP[r]) <= eSP[r] * Fraction(1, 2 ** 50)
    assert not np.any(s[2]) and not np.any(S[2])
    print("\nweighted_sums against Fraction: worst {:.3g} units".format(worst))
    assert worst <= 0.1


# ---------------------------------------------------------------------------------------------------------------------------
# the conditions the tables satisfy without the device
# ---------------------------------------------------------------------------------------------------------------------------
def test_xcov_table_holds_what_it_claims():
    """every case: the counts are a direct NumPy count, no scale is zero where the reference value is not, and the hand-placed
    samples are there: exact zeros in the one-sample pair level, a zero row and column, the (1, 0, 0, 1) pair, NaNs at the
    batch edges, the level without a kept sample; the sizes cover each band's boundaries"""
    cases = gc.xcov_cases()
    seen_sizes = {}
    for case in cases.values():
        ref, M = gc.xcov_reference(case), case.M
        a = np.zeros(M) if case.shift is None else case.shift
        for l, (f, c) in enumerate(case.levels):
            n = f.shape[1]
            bad = np.isnan(f).any(axis=0) | (False if c is None else np.isnan(c).any(axis=0))
            assert ref.n[l] == n - bad.sum() and ref.n_rm[l] == bad.sum(), (case, l)
            for v, sc in ((ref.s[l], ref.S[l]), (ref.sp[l], ref.SP[l])):
                assert np.all(np.isfinite(v.astype(np.float64))) and np.all(v[sc == 0] == 0), (case, l)
            seen_sizes.setdefault((M, c is not None), set()).add(n)
            if case.name.startswith("m") and "level0" not in case.name:
                z = gc.zero_component(M)
                S = ref.S[l].reshape(M, M)
                if z is not None and ref.n[l] > 0:
                    assert not np.any(S[z]) and not np.any(S[:, z]) and np.all(np.delete(np.diag(S), z) > 0), (case, l)
                if n == 1 and c is not None:
                    assert ref.n[l] == 1 and not np.any(ref.s[l]) and not np.any(ref.sp[l]) and np.any(ref.S[l] > 0), (case, l)
                if n >= 8 and c is not None and M >= 2:
                    j = M - 1
                    assert (f[0, 3] - a[0], c[0, 3] - a[0], f[j, 3] - a[j], c[j, 3] - a[j]) == (1.0, 0.0, 0.0, 1.0)
                    assert (f[0, 4] - a[0], c[0, 4] - a[0], f[j, 4] - a[j], c[j, 4] - a[j]) == (0.0, 1.0, 1.0, 0.0)
                    assert not bad[2] and not bad[3] and not bad[4] and np.array_equal(f[:, 2], c[:, 2])
                if n >= 8:
                    B = gc.xcov_batch(M)
                    assert bad[0] and bad[n - 1] and (n <= B or bad[B - 1]) and (n <= B + 1 or bad[B]), (case, l)
                    if c is not None and n > B + 1:
                        assert np.isnan(f[0, 0]) and not np.isnan(c[:, 0]).any() and np.isnan(c[0, B]) and not np.isnan(f[:, B]).any()
                    if M > 64:
                        assert np.isnan(f[gc.later_component(M), 5])
    for M in gc.XCOV_M:
        assert seen_sizes[M, True] >= set(gc.xcov_level_sizes(M)) and seen_sizes[M, False] >= set(gc.xcov_level_sizes(M)), M
    for name in ("alldrop_5", "alldrop_70"):
        ref = gc.xcov_reference(cases[name])
        assert ref.n[1] == 0 and ref.n_rm[1] == 40 and not np.any(ref.s[1]) and not np.any(ref.S[1]) and ref.n[0] > 0 and ref.n[2] > 0
    ref = gc.xcov_reference(cases["scales_17"])
    S = ref.S[0].reshape(17, 17)
    assert S[16, 16] / S[0, 0] > 1e22
    # shift None: the zero component holds both signed zeros
    f = cases["m17_level0_65"].levels[0][0][gc.zero_component(17)]
    assert np.any(np.signbit(f) & (f == 0)) and np.any(~np.signbit(f) & (f == 0))
    assert set(cases["m1024"].levels[l][0].shape[1] for l in range(2)) == {40, 3}


def test_boot_table_holds_what_it_claims():
    """every case: the kept counts of the reference under NumPy's multinomial weights equal a direct count, no scale is zero where
    the value is not, a replicate of no picks has zero sums, and the chunks hold dropped samples at the cut positions; the
    tables cover the sizes, replicate counts and column counts asked for"""
    ns, Bs, shared_cols, comp_shapes = set(), set(), set(), set()
    for case in gc.boot_cases().values():
        w = gc.multinomial_weights(case)
        n, s, sp, S, SP = gc.boot_sums(case, w)
        direct = np.zeros_like(n)
        for i, call in enumerate(case.calls):
            keep = gc.boot_keeps(case, call)                                      # [G, n]
            direct[:, call[0], :] += (w[i][:, None, :] * keep[None, :, :]).sum(axis=-1)
            nn = call[1].shape[1]
            ns.add(nn)
            if nn >= 8:
                for pos in [p for p in gc.EDGES + (nn - 1,) if p < nn]:
                    assert not keep[:, pos].all(), (case, i, pos)
            assert call[3][-1] == nn and np.all(call[3] <= nn) and (case.B <= 15 or call[3][15] == 0)
            assert (call[2] is None) == (call[0] == 0)
            if call[0] == 2:
                assert nn == 1 and keep.all(), case                                # the one-sample level is kept
        assert np.array_equal(n, direct), case
        for v, sc in ((s, S), (sp, SP)):
            assert np.all(np.isfinite(v.astype(np.float64))) and np.all(v[sc == 0] == 0), case
        if 15 in case.checked:
            k = case.checked.index(15)
            assert not np.any(n[k]) and not np.any(S[k]) and not np.any(s[k])
        Bs.add(case.B)
        if case.layout == "shared":
            shared_cols.add(case.M * case.K)
        else:
            comp_shapes.add((case.K, case.M))
            assert len({d.domain for d in case.descs}) == min(case.M, 3 if case.descs[0].log else 4)
    assert ns >= {1, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 9001, 32769, 40000}
    assert Bs == {1, 17, 70, 257}
    assert shared_cols >= {1, 16, 17, 32, 33, 35, 64, 65, 130}
    assert {k for k, _ in comp_shapes} >= {7, 15, 16, 60} and {m for _, m in comp_shapes} >= {1, 5, 40}
    # a chunk in which every sample (of a component) is dropped
    for name, g in (("s35", 0), ("c15_40", 1)):
        case = gc.boot_cases()[name]
        assert not gc.boot_keeps(case, case.calls[1])[g].any()


# ---------------------------------------------------------------------------------------------------------------------------
# the twins
# ---------------------------------------------------------------------------------------------------------------------------
def _two_digits(measured, recorded):
    if recorded is None or measured is None:
        return recorded is None and measured is None
    return abs(measured - recorded) <= 0.01 * recorded + 1e-3


def calibrate_xcov():
    """{class: {quantity: [A, B]}}, {(class, quantity, variant): "case level l"}"""
    table, where = {}, {}
    for case in gc.xcov_cases().values():
        ref = gc.xcov_reference(case)
        for vi, variant in enumerate("AB"):
            twin = gx.xcov_sums(case.levels, case.shift, np.float64, variant)
            assert np.array_equal(twin.n, ref.n) and np.array_equal(twin.n_rm, ref.n_rm)
            for l, (f, c) in enumerate(case.levels):
                cls = gc.xcov_class(case.M, c is not None)
                for q, got, want, scale in (("s", twin.s[l], ref.s[l], ref.S[l]), ("sp", twin.sp[l], ref.sp[l], ref.SP[l])):
                    w, _ = ax.worst(got, want, scale)
                    assert np.isfinite(w), (case, l, q, variant)              # exact zeros where the scale is zero
                    row = table.setdefault(cls, {}).setdefault(q, [0.0, 0.0])
                    if w >= row[vi]:
                        row[vi] = w
                        where[cls, q, variant] = "{} level {}".format(case.name, l)
    return table, where


def _has_b(desc):
    return desc.kind in (ax.LEGENDRE, ax.FOURIER)


def calibrate_boot():
    table, where = {}, {}
    for case in gc.boot_cases().values():
        w = gc.multinomial_weights(case)
        n, s, sp, S, SP = gc.boot_sums(case, w)
        for vi, variant in enumerate(("A", "B") if _has_b(case.descs[0]) else ("A",)):
            tn, ts, tsp, _, _ = gc.boot_sums(case, w, np.float64, variant)
            assert np.array_equal(tn, n)
            for q, got, want, scale in (("s", ts, s, S), ("sp", tsp, sp, SP)):
                u, _ = ax.worst(got, want, scale)
                assert np.isfinite(u), (case, q, variant)
                row = table.setdefault(case.cls, {}).setdefault(q, [0.0, 0.0 if _has_b(case.descs[0]) else None])
                if u >= row[vi]:
                    row[vi] = u
                    where[case.cls, q, variant] = case.name
    return table, where


def _show_and_check(table, where, recorded, tolerance):
    print()
    for cls in sorted(table):
        for q, (a, b) in table[cls].items():
            print("{:16s} {:3s} twin A {:9.4g} ({})  twin B {}  tolerance {:.4g}".format(
                cls, q, a, where[cls, q, "A"], "{:9.4g} ({})".format(b, where[cls, q, "B"]) if b is not None else "        -",
                max(16.0, 4 * max(a, b or 0.0))))
    assert set(table) == set(recorded), (sorted(table), sorted(recorded))
    for cls in table:
        assert set(table[cls]) == set(recorded[cls]), cls
        for q, (a, b) in table[cls].items():
            ra, rb = recorded[cls][q]
            assert _two_digits(a, ra) and _two_digits(b, rb), (cls, q, a, b, ra, rb)
            assert tolerance(cls, q) == max(16.0, 4.0 * max(ra, rb or 0.0))


def test_xcov_twin_calibration_table():
    """both twins on every level of every case: the worst units per class are the recorded XCOV_TWIN_UNITS to two digits"""
    table, where = calibrate_xcov()
    _show_and_check(table, where, gc.XCOV_TWIN_UNITS, gc.xcov_tolerance)


def test_boot_twin_calibration_table():
    """the weighted twins on every case: the worst units per class are the recorded BOOT_TWIN_UNITS to two digits"""
    table, where = calibrate_boot()
    _show_and_check(table, where, gc.BOOT_TWIN_UNITS, gc.boot_tolerance)


# ---------------------------------------------------------------------------------------------------------------------------
# what the gates catch: deliberately broken twins
# ---------------------------------------------------------------------------------------------------------------------------
WIDE = 100.0                                          # every flaw exceeds the gate of its class by this factor at least


def _xcov_level_units(case, l, s, sp):
    ref = gc.xcov_reference(case)
    return ax.worst(s.reshape(-1), ref.s[l], ref.S[l])[0], ax.worst(sp.reshape(-1), ref.sp[l], ref.SP[l])[0]


@pytest.mark.parametrize("name,l", [("m16", 5), ("m33", 1), ("m129", 5), ("m129", 0)])
def test_a_sample_dropped_at_a_batch_edge_is_caught(name, l):
    """the identities in fp64 without sample B (the first of the second batch) of the kept samples"""
    case = gc.xcov_cases()[name]
    f, c = case.levels[l]
    keep, F, C = gx.xcov_kept(f, c, case.shift)
    k = gc.xcov_batch(case.M)
    assert F.shape[1] > k + 1
    cls = gc.xcov_class(case.M, c is not None)
    sound = _xcov_level_units(case, l, *gx.xcov_identities(F, C))
    assert sound[0] <= gc.xcov_tolerance(cls, "s") and sound[1] <= gc.xcov_tolerance(cls, "sp")
    us, usp = _xcov_level_units(case, l, *gx.xcov_identities(np.delete(F, k, axis=1), None if C is None else np.delete(C, k, axis=1)))
    print("\n{} level {}: a dropped sample gives {:.3g} / {:.3g} units (gates {:.3g} / {:.3g})".format(
        name, l, us, usp, gc.xcov_tolerance(cls, "s"), gc.xcov_tolerance(cls, "sp")))
    assert us > WIDE * gc.xcov_tolerance(cls, "s") and usp > WIDE * gc.xcov_tolerance(cls, "sp")


@pytest.mark.parametrize("name,l", [("m16", 5), ("m65", 1), ("m32", 0)])
def test_a_dropped_sample_with_a_small_term_passes_the_first_gate_only(name, l):
    """The same flaw on a sample 1e-4 the size of the others: its term is 1e-8 of one ordinary term, inside the 1e-10 of
    sum (|f_i f_j| + |c_i c_j|) that tests/test_gpu_component_cov.py grants the means, and still far outside the gate of s."""
    case = gc.xcov_cases()[name]
    f, c = case.levels[l]
    _, F, C = gx.xcov_kept(f, c, case.shift)
    k = gc.xcov_batch(case.M)
    F = F.copy()
    F[:, k] *= 1e-4
    if C is not None:
        C = C.copy()
        C[:, k] *= 1e-4
    s, _, S, _ = gx.xcov_definition(F, C)
    flawed, _ = gx.xcov_identities(np.delete(F, k, axis=1), None if C is None else np.delete(C, k, axis=1))
    first = 1e-10 * (np.abs(F) @ np.abs(F).T + (0 if C is None else np.abs(C) @ np.abs(C).T))
    z = gc.zero_component(case.M)
    live = np.ones(case.M, dtype=bool)
    live[z] = False
    err = np.abs(flawed - s.astype(np.float64))
    assert np.all(err <= first) and np.any(err[np.ix_(live, live)] > 0)
    cls = gc.xcov_class(case.M, c is not None)
    units = ax.worst(flawed, s, S)[0]
    print("\n{} level {}: {:.3g} units (gate {:.3g}), {:.3g} of the first gate".format(
        name, l, units, gc.xcov_tolerance(cls, "s"), float(np.max(err[np.ix_(live, live)] / first[np.ix_(live, live)]))))
    assert units > WIDE * gc.xcov_tolerance(cls, "s")


@pytest.mark.parametrize("name,l", [("m200", 1), ("m129", 1), ("m129", 0)])
def test_the_mirror_tile_of_an_off_diagonal_block_is_caught(name, l):
    """block (0, 1) of the 64-wide tiling stored untransposed -- the tile of its mirror (1, 0): a wrong lane-to-tile mapping of
    the C / D registers.  The result stays symmetric; only the reference sees it."""
    case = gc.xcov_cases()[name]
    f, c = case.levels[l]
    _, F, C = gx.xcov_kept(f, c, case.shift)
    s, sp = gx.xcov_identities(F, C)
    for v in (s, sp):
        blk = v[0:64, 64:128].copy()
        v[0:64, 64:128] = blk.T
        v[64:128, 0:64] = blk
        assert np.array_equal(v, v.T)
    cls = gc.xcov_class(case.M, c is not None)
    us, usp = _xcov_level_units(case, l, s, sp)
    assert us > WIDE * gc.xcov_tolerance(cls, "s") and usp > WIDE * gc.xcov_tolerance(cls, "sp"), (us, usp)


@pytest.mark.parametrize("name", ["m2", "m17", "m64", "m200", "scales_17"])
def test_v1_plus_v2_is_caught(name):
    """sp = 1/4 (G1 + G1^T + G2) in place of 1/4 (G1 + G1^T + 2 G2) on the pair levels with more than one kept sample: the two
    agree only where d or s vanishes"""
    case = gc.xcov_cases()[name]
    ref = gc.xcov_reference(case)
    hit = 0
    for l, (f, c) in enumerate(case.levels):
        if c is None or ref.n[l] < 2:
            continue
        _, F, C = gx.xcov_kept(f, c, case.shift)
        us, usp = _xcov_level_units(case, l, *gx.xcov_identities(F, C, g2_weight=1.0))
        cls = gc.xcov_class(case.M, True)
        assert us <= gc.xcov_tolerance(cls, "s") and usp > WIDE * gc.xcov_tolerance(cls, "sp"), (name, l, us, usp)
        hit += 1
    assert hit >= 1


def test_weights_one_sample_off_at_a_range_start_are_caught():
    """the weight rows of the second 32768-sample range read one sample late"""
    for name in ("s17", "c7_5"):                          # 40000 samples: 7232 of them in the second range
        case = gc.boot_cases()[name]
        w = gc.multinomial_weights(case)
        n, s, sp, S, SP = gc.boot_sums(case, w)
        flawed = [x.copy() for x in w]
        assert flawed[0].shape[1] > 32768
        flawed[0][:, 32769:] = w[0][:, 32768:-1]
        flawed[0][:, 32768] = 0
        _, ts, tsp, _, _ = gc.boot_sums(case, flawed, np.float64)
        live = [k for k, b in enumerate(case.checked) if case.calls[0][3][b] > 0]
        us, usp = ax.worst(ts[live, 0], s[live, 0], S[live, 0])[0], ax.worst(tsp[live, 0], sp[live, 0], SP[live, 0])[0]
        print("\n{}: shifted weights give {:.3g} / {:.3g} units (gates {:.3g} / {:.3g})".format(
            name, us, usp, gc.boot_tolerance(case.cls, "s"), gc.boot_tolerance(case.cls, "sp")))
        assert us > WIDE * gc.boot_tolerance(case.cls, "s") and usp > WIDE * gc.boot_tolerance(case.cls, "sp")


def test_the_flag_column_summed_into_d0_is_caught():
    """per-component layout: the keep flag of a component added into its first term"""
    for name in ("c7_1", "c16_5", "c15_40", "clog"):
        case = gc.boot_cases()[name]
        w = gc.multinomial_weights(case)
        n, s, sp, S, SP = gc.boot_sums(case, w)
        _, ts, _, _, _ = gc.boot_sums(case, w, np.float64)
        ts[..., 0] += n
        live = [k for k, b in enumerate(case.checked) if case.calls[0][3][b] > 0]
        for level in (0, 1):
            us = ax.worst(ts[live, level], s[live, level], S[live, level])[0]
            assert us > WIDE * gc.boot_tolerance(case.cls, "s"), (name, level, us)
