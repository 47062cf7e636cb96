"""CPU checks of the extended-precision reference of the moment covariance (tests/cov_exact.py): the reference against exact
rational arithmetic on the same rounded rows, the conditions the case table of tests/cov_cases.py must satisfy without a device,
the calibration of the fp64 twins (printed with pytest -s, pinned by COV_TWIN_UNITS, from which tests/test_gpu_cov_exact.py
derives the device tolerances), deliberately broken twins that show what the gates catch, and the new tolerances rewritten in the
form of the gates that held the covariance routes before (1e-10, 1e-11, 1e-12 of sqrt(|sp| n))."""
from fractions import Fraction

import numpy as np
import pytest

from tests import accum_exact as ax
from tests import cov_cases as cc
from tests import cov_exact as cx
from tests import gram_exact as gx
from tests.test_gram_exact_cpu import _frac, _two_digits, _units

LD = np.longdouble
WIDE = 100.0                                          # a flaw "caught with room" exceeds the gate of its class by this factor


def test_long_double_is_extended_precision():
    """without an 80-bit long double the module proves nothing: a failure, not a skip"""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


# ---------------------------------------------------------------------------------------------------------------------------
# the reference against exact rational arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
def _exact_rows(desc, t):
    p = [Fraction(1), t]
    for i in range(2, desc.size):
        p.append(((2 * i - 1) * t * p[i - 1] - (i - 1) * p[i - 2]) / i if desc.kind == ax.LEGENDRE else p[i - 1] * t)
    return p[:desc.size]


@pytest.mark.parametrize("kind", [ax.LEGENDRE, ax.MONOMIAL])
def test_cov_sums_against_fractions(kind):
    """R = 4, 14 samples, a level without coarse values and a pair level (one pair with fine == coarse, dropped samples), with
    and without a 3 x 4 matrix: s, sp within 0.1 unit of the exact sums of the rows at the same fp64 t; the scales to 2^-50"""
    rng = np.random.default_rng(3)
    R, n = 4, 14
    desc = ax.Desc(kind, R, (-3.0, 3.5), (0.0, 1.0) if kind == ax.MONOMIAL else None)
    f = rng.normal(size=(1, n))
    c = f + 0.1 * rng.normal(size=(1, n))
    f[0, 3], c[0, 11], f[0, 13], c[0, 5] = np.nan, 9.0, -3.5, f[0, 5]
    levels = [(f.copy(), None), (f, c)]
    T = rng.normal(size=(3, R))
    worst = 0.0
    for matrix in (None, T):
        ref = cx.cov_sums(desc, levels, matrix=matrix)
        Ro = R if matrix is None else 3
        Tf = [[Fraction(float(v)) for v in row] for row in (np.eye(R) if matrix is None else matrix)]
        assert list(ref.n) == [n - 2, n - 3] and list(ref.n_rm) == [2, 3]
        for l, (fl, cl) in enumerate(levels):
            tf, kf, _ = ax.transform(desc, fl[0], np.float64)
            keep = kf if cl is None else kf & ax.transform(desc, cl[0], np.float64)[1]
            tc = None if cl is None else ax.transform(desc, cl[0], np.float64)[0]
            es, esp, eS, eSP = ([[Fraction(0)] * Ro for _ in range(Ro)] for _ in range(4))
            for k in np.flatnonzero(keep):
                pf = _exact_rows(desc, Fraction(float(tf[k])))
                pc = [Fraction(0)] * R if tc is None else _exact_rows(desc, Fraction(float(tc[k])))
                a = [abs(x) + abs(y) for x, y in zip(pf, pc)]
                qf = [sum(Tf[i][r] * pf[r] for r in range(R)) for i in range(Ro)]
                qc = [sum(Tf[i][r] * pc[r] for r in range(R)) for i in range(Ro)]
                qa = [sum(abs(Tf[i][r]) * a[r] for r in range(R)) for i in range(Ro)]
                for i in range(Ro):
                    for j in range(Ro):
                        y, A = qf[i] * qf[j] - qc[i] * qc[j], qa[i] * qa[j]
                        es[i][j] += y
                        esp[i][j] += y * y
                        eS[i][j] += A
                        eSP[i][j] += A * A
            for i in range(Ro):
                for j in range(Ro):
                    e = i * Ro + j
                    worst = max(worst, _units(ref.s[l, e], es[i][j], eS[i][j]), _units(ref.sp[l, e], esp[i][j], eSP[i][j]))
                    assert abs(_frac(ref.S[l, e]) - eS[i][j]) <= eS[i][j] * Fraction(1, 2 ** 50)
                    assert abs(_frac(ref.SP[l, e]) - eSP[i][j]) <= eSP[i][j] * Fraction(1, 2 ** 50)
    print("\ncov_sums ({}) against Fraction: worst {:.3g} units".format(kind, worst))
    assert worst <= 0.1


def test_diff_gram_sums_against_fractions():
    """the difference Gram of TransformedMoments, R = 4 -> 3 rows, on the same exact rows"""
    rng = np.random.default_rng(4)
    R, n = 4, 10
    desc = ax.Desc(ax.LEGENDRE, R, (-3.0, 3.5))
    f = rng.normal(size=(1, n))
    c = f + 0.1 * rng.normal(size=(1, n))
    f[0, 2] = np.nan
    T = rng.normal(size=(3, R))
    ref = cx.diff_gram_sums(desc, [(f, c)], T)
    tf, kf, _ = ax.transform(desc, f[0], np.float64)
    tc, kc, _ = ax.transform(desc, c[0], np.float64)
    worst = 0.0
    for i in range(3):
        es = esp = eS = eSP = Fraction(0)
        for k in np.flatnonzero(kf & kc):
            pf, pc = _exact_rows(desc, Fraction(float(tf[k]))), _exact_rows(desc, Fraction(float(tc[k])))
            d = sum(Fraction(float(T[i, r])) * (pf[r] - pc[r]) for r in range(R))
            b = sum(abs(Fraction(float(T[i, r]))) * (abs(pf[r]) + abs(pc[r])) for r in range(R))
            es, esp, eS, eSP = es + d, esp + d * d, eS + b, eSP + b * b
        worst = max(worst, _units(ref.s[0, i], es, eS), _units(ref.sp[0, i], esp, eSP))
    assert list(ref.n) == [n - 1] and worst <= 0.1, worst


# ---------------------------------------------------------------------------------------------------------------------------
# the conditions the table satisfies without the device
# ---------------------------------------------------------------------------------------------------------------------------
def test_batches_are_those_of_the_code():
    """the batch and grid sizes come out of cov.hip; the table of the issue is what they give today"""
    k = cc.kernel_constants()
    assert k == {"t4_batch": 32, "wide_batch": 32, "t4_wgs": 4}, k
    assert [cc.batches(x) for x in ("t1", "t2", "t4", "wide", "vals")] == [(128, 256), (128, 256), (32, 64), (32, 64), (64, 64)]
    assert [cc.kernel_of(R) for R in (1, 16, 17, 32, 33, 64, 65, 128, 129)] == ["t1", "t1", "t2", "t2", "t4", "t4", "wide", "wide", "vals"]


def test_table_holds_what_it_claims():
    """every case: counts are a direct count, values finite, no scale is zero where the value is not; the level sizes are
    1, B - 1, B, B + 1, 4 B + 3 of the case's kernel with and without coarse values, with dropped samples at 0, B - 1, B, n - 1 in
    one member only; the one-sample pair level is fine == coarse and exactly zero; an independent pair level per band; the long
    levels exceed a full grid by more than a batch; one level is dropped entirely; the spline zeros are exact"""
    cases = cc.cases()
    bands_indep = set()
    for case in cases.values():
        ref = cc.reference(case)
        Bp, B0 = cc.batches(case.kernel)
        sizes = {True: set(), False: set()}
        for l, (f, c) in enumerate(case.levels):
            n = f.shape[1]
            keep = cx.kept_rows(cx.extended(case.desc, 1), f, c, np.float64)[0]
            assert ref.n[l] == keep.sum() and ref.n_rm[l] == n - keep.sum(), (case, l)
            sizes[c is not None].add(n)
            for v, sc in ((ref.s[l], ref.S[l]), (ref.sp[l], ref.SP[l])):
                assert np.all(np.isfinite(v.astype(np.float64))) and np.all(v[sc == 0] == 0), (case, l)
            if case.name.startswith(("legendre_", "fourier_", "spline_", "monomial_", "log_", "transformed_", "diffgram_")):
                B = Bp if c is not None else B0
                drops = cc.drop_positions(n, B)
                assert not keep[drops].any(), (case, l, drops)
                if c is not None and n >= 8:
                    only_f = [p for p in drops if not ax.transform(case.desc, f[:, p], np.float64)[1].all()
                              and ax.transform(case.desc, c[:, p], np.float64)[1].all()]
                    only_c = [p for p in drops if ax.transform(case.desc, f[:, p], np.float64)[1].all()
                              and not ax.transform(case.desc, c[:, p], np.float64)[1].all()]
                    assert only_f and only_c, (case, l)
                if c is not None and n == 1:
                    assert f[0, 0] == c[0, 0] and ref.n[l] == 1 and not np.any(ref.s[l]) and not np.any(ref.sp[l]) and np.any(ref.S[l] > 0)
                if c is not None and n == 2 * Bp + 1:                   # the independent draw: |f - c| of the order of the values
                    assert np.nanmedian(np.abs(f - c)) > 0.3 * np.nanmedian(np.abs(f)), (case, l)
                    bands_indep.add(case.band)
        if case.name.startswith(("fourier_", "spline_", "monomial_", "log_")) or case.name in ["legendre_{}".format(R) for R in cc.FULL_R]:
            assert sizes[True] >= {1, Bp - 1, Bp, Bp + 1, 4 * Bp + 3} and sizes[False] >= {1, B0 - 1, B0, B0 + 1, 4 * B0 + 3}, case
        if case.name.startswith("long_"):
            n = case.levels[0][0].shape[1]
            assert n > cc.grid(case.kernel) * Bp + Bp and n % Bp, case
    assert bands_indep >= {"legendre<=16", "legendre<=32", "legendre<=64", "legendre<=128", "legendre<=256", "fourier", "monomial",
                           "log", "spline8", "spline37", "spline128", "transformed", "transformed>128"}
    assert {cases["long_{}_{}".format(k, R)].kernel for k, R in cc.LONG_R.items()} | {cases["long_vals_8x16"].kernel} == \
        {"t1", "t2", "t4", "wide", "vals"}
    ref = cc.reference(cases["alldrop_33"])
    assert ref.n[1] == 0 and ref.n_rm[1] == 40 and not np.any(ref.s[1]) and not np.any(ref.S[1]) and ref.n[0] > 0 and ref.n[2] > 0
    for name, M in (("vector2_49", 2), ("vector3_17", 3)):              # NaNs in one component only, one shared mask
        f, c = cases[name].levels[1]
        alone = (np.isnan(f).sum(axis=0) + np.isnan(c).sum(axis=0)) == 1
        assert f.shape[0] == M and alone.sum() >= 8 and np.isnan(f[0]).any() and np.isnan(c[M - 1]).any()
    for R in cc.SPLINE_R:                                               # no common support: an exact zero is demanded
        ref = cc.reference(cases["spline_{}".format(R)])
        I, J = np.meshgrid(np.arange(R), np.arange(R), indexing="ij")
        far = ((np.abs(I - J) > 3) & (I >= 1) & (J >= 1)).reshape(-1)
        l0 = [l for l, (f, c) in enumerate(cases["spline_{}".format(R)].levels) if c is None]   # (a pair whose members lie in
        # distant knot spans has cross terms |B_i(f)| |B_j(c)| in its scale: the zeros are those of the levels without coarse values)
        # (a value on a knot: the long-double v = u ns lies ~1e-15 into the span before the one fp64 finds -- a tiny scale, not 0)
        assert far.any() and not np.any(ref.s[l0][:, far]) and np.all(ref.S[l0][:, far] < 1e-12) and np.all(ref.SP[l0][:, far] < 1e-24)
        assert np.mean(ref.S[l0][:, far] == 0) > (0.99 if R > 8 else 0.8)
        assert R > 8 or np.all(ref.S[4][~far] > 0)
    # every route of the issue is named in some case
    assert {r for case in cases.values() for r in case.routes} == set(cc.ROUTES)
    assert cc.lin_eligible(cases["monomial_33"].desc) and not cc.lin_eligible(cases["unclipped_20"].desc)


# ---------------------------------------------------------------------------------------------------------------------------
# the twins
# ---------------------------------------------------------------------------------------------------------------------------
def _has_b(desc):
    return desc.kind in (ax.LEGENDRE, ax.FOURIER)


def lin_twins(case, squares):
    """the fp64 emulations of a linearised entry, each [L, M * R * R]: (A, B) = (extended Legendre / monomial level sums of
    accum_exact, both row variants, contracted in ascending k; the route's own recurrences | None for monomials: Legendre sums by
    the matrix kernel's scaled monic recurrence; Chebyshev sums with the second window started by doubling; at 49..64 moments the
    first 64 Chebyshev sums from the monic Legendre sums through the connection table) -- lists of named candidates per twin; the calibration table prints which one sets a figure"""
    d, R = case.desc, case.desc.size
    K = 4 * R - 3 if squares else 2 * R - 1
    table = cc.lib_table(d, squares)
    a = []
    for variant in ("A", "B") if d.kind == ax.LEGENDRE else ("A",):
        ext = ax.level_sums(cx.extended(d, K), case.levels, np.float64, variant)
        a.append(("rows " + variant, cx.lin_contract(table, ext.s.reshape(case.L, case.M, K)).reshape(case.L, -1)))
    b = []
    if d.kind == ax.LEGENDRE:
        monic = cx.route_level_sums(d, case.levels, K, cx.legendre_monic_sums)
        b.append(("monic Legendre sums", cx.lin_contract(table, monic).reshape(case.L, -1)))
        cheb_table = cc.lib_table(d, squares + 2)
        cheb = cx.route_level_sums(d, case.levels, K, cx.chebyshev_sums)
        b.append(("Chebyshev sums", cx.lin_contract(cheb_table, cheb).reshape(case.L, -1)))
        if 49 <= R <= 64 and not squares:
            rows = cheb.copy()
            rows[..., :64] = np.einsum("mk,lck->lcm", cc.lib_connection(64), monic[..., :64])
            b.append(("row sums through the connection", cx.lin_contract(cheb_table, rows).reshape(case.L, -1)))
    return a, b


def calibrate():
    """{class key: [A, B]}, {(key, twin): place}, {R: worst ratio of the linearised to the definitional scale of sp}"""
    table, where, ratios = {}, {}, {}

    def note(key, vi, units, place, has_b=True):
        assert np.isfinite(units), (key, vi, place)                       # exact zeros where the scale is zero
        row = table.setdefault(key, [0.0, 0.0 if has_b else None])
        if row[vi] is None or units >= row[vi]:
            row[vi] = units
            where[key, vi] = place

    for case in cc.cases().values():
        ref = cc.reference(case)
        has_b = _has_b(case.desc)
        if case.entry == "diff":
            twins = [cx.diff_gram_sums(case.desc, case.levels, case.matrix, np.float64, v) for v in "AB"]
        else:
            twins = [cx.cov_sums(case.desc, case.levels, np.float64, "A", matrix=case.matrix),
                     cx.cov_sums(case.desc, case.levels, np.float64, "B" if has_b else "A", identities=True, matrix=case.matrix)]
        for vi, twin in enumerate(twins):
            assert np.array_equal(twin.n, ref.n) and np.array_equal(twin.n_rm, ref.n_rm)
            for l in range(case.L):
                for q in ("s", "sp"):
                    key, want, scale = cc.judged(case, "direct", l, q)
                    note(key, vi, ax.worst(getattr(twin, q)[l], want, scale)[0], "{} level {}".format(case.name, l))
        if not any(r.startswith("lin") for r in case.routes) or not cc.lin_eligible(case.desc, case.matrix):
            continue
        for q, squares in (("s", 0), ("sp", 1)):
            if q == "sp" and (case.desc.size > 64 or all(c is not None for _, c in case.levels)):
                continue                                                  # no level whose second moments are linearised
            for vi, cands in enumerate(lin_twins(case, squares)):
                for cname, got in cands:
                    for l, (f, c) in enumerate(case.levels):
                        if q == "sp" and c is not None:
                            continue
                        key, want, scale = cc.judged(case, "lin", l, q)
                        assert key[1] == "lin"
                        note(key, vi, ax.worst(got[l], want, scale)[0], "{} level {}, {}".format(case.name, l, cname), case.desc.kind == ax.LEGENDRE)
                        if q == "sp" and ref.n[l] > 1:
                            live = ref.SP[l] > 0
                            ratios[case.desc.kind, case.desc.size] = max(ratios.get((case.desc.kind, case.desc.size), 0.0),
                                                                         float(np.max(scale[live] / ref.SP[l][live])))
    return table, where, ratios


@pytest.fixture(scope="module")
def calibration():
    return calibrate()


def test_twin_calibration_table(calibration):
    """both twins on every level of every case: the worst units per class are the recorded COV_TWIN_UNITS to two digits"""
    table, where, ratios = calibration
    print()
    for key in sorted(table):
        a, b = table[key]
        print("{:18s} {:6s} {:4s} {:2s} twin A {:9.4g} ({})  twin B {}  tolerance {:.4g}".format(
            *key, a, where[key, 0], "{:9.4g} ({})".format(b, where[key, 1]) if b is not None else "        -", max(16.0, 4 * max(a, b or 0.0))))
    print("linearised / definitional scale of the second moments without coarse values, worst entry:",
          {"{}{}".format(*k): "{:.3g}".format(v) for k, v in sorted(ratios.items())})
    assert set(table) == set(cc.COV_TWIN_UNITS), (sorted(set(table) ^ set(cc.COV_TWIN_UNITS)))
    for key, (a, b) in table.items():
        ra, rb = cc.COV_TWIN_UNITS[key]
        assert _two_digits(a, ra) and _two_digits(b, rb), (key, a, b, ra, rb)
        assert cc.tolerance(key) == max(16.0, 4.0 * max(ra, rb or 0.0))


# ---------------------------------------------------------------------------------------------------------------------------
# what the gates catch: deliberately broken twins
# ---------------------------------------------------------------------------------------------------------------------------
def _rows(case, l, variant="B"):
    """fp64 rows F, C | None [R, n_keep] of component 0 of a level"""
    f, c = case.levels[l]
    _, pf, pc, _ = cx.kept_rows(case.desc, f, c, np.float64, variant if _has_b(case.desc) else "A")
    return pf[0], None if pc is None else pc[0]


def _level_units(case, l, s, sp):
    out = []
    for q, v in (("s", s), ("sp", sp)):
        key, want, scale = cc.judged(case, "direct", l, q)
        out.append(ax.worst(v.reshape(-1), want, scale)[0] / cc.tolerance(key))
    return out


def _level_of(case, n, pair):
    return [l for l, (f, c) in enumerate(case.levels) if f.shape[1] == n and (c is not None) == pair][0]


@pytest.mark.parametrize("name", ["legendre_5", "legendre_17", "legendre_64", "legendre_100", "legendre_129", "fourier_33", "spline_37"])
@pytest.mark.parametrize("pair", [False, True])
def test_a_sample_dropped_at_a_batch_edge_is_caught(name, pair):
    """the identities in fp64 without kept sample B (the first of the second batch) of the level of 4 B + 3 samples"""
    case = cc.cases()[name]
    B = cc.batches(case.kernel)[0 if pair else 1]
    l = _level_of(case, 4 * B + 3, pair)
    F, C = _rows(case, l)
    sound = _level_units(case, l, *gx.xcov_identities(F, C))
    assert max(sound) <= 1.0, sound
    us, usp = _level_units(case, l, *gx.xcov_identities(np.delete(F, B, axis=1), None if C is None else np.delete(C, B, axis=1)))
    print("\n{} level {}: a dropped sample exceeds the gates of s / sp {:.3g} / {:.3g} times".format(name, l, us, usp))
    assert us > WIDE and usp > WIDE


@pytest.mark.parametrize("name", ["legendre_17", "legendre_64", "legendre_100"])
@pytest.mark.parametrize("pair", [False, True])
def test_a_dropped_small_sample_passes_the_old_gate_only(name, pair):
    """The same flaw on a sample whose rows are 1e-4 the size of the others (its terms are 1e-8 and 1e-16 of an ordinary one):
    inside 1e-10 of max(|s|, sqrt(|sp| n)) and of |sp| in every entry, and still outside the new gate of s."""
    case = cc.cases()[name]
    B = cc.batches(case.kernel)[0 if pair else 1]
    l = _level_of(case, 4 * B + 3, pair)
    F, C = _rows(case, l)
    F = F.copy()
    F[:, B] *= 1e-4
    if C is not None:
        C = C.copy()
        C[:, B] *= 1e-4
    a = np.abs(F) + (0 if C is None else np.abs(C))
    s, sp, S, SP = cx.definition(F, C, a)
    fs, fsp = gx.xcov_identities(np.delete(F, B, axis=1), None if C is None else np.delete(C, B, axis=1))
    n = F.shape[1]
    old_s = 1e-10 * np.maximum(np.abs(s), np.sqrt(np.abs(sp) * n)).astype(np.float64)
    assert np.all(np.abs(fs - s.astype(np.float64)) <= old_s) and np.all(np.abs(fsp - sp.astype(np.float64)) <= 1e-10 * np.abs(sp).astype(np.float64) + 1e-13)
    key = cc.judged(case, "direct", l, "s")[0]
    units = ax.worst(fs, s, S)[0] / cc.tolerance(key)
    print("\n{} level {}: the small sample exceeds the gate of s {:.3g} times".format(name, l, units))
    assert units > WIDE


@pytest.mark.parametrize("name", ["legendre_17", "legendre_64", "legendre_100", "legendre_129", "monomial_33"])
def test_g1_plus_g2_is_caught(name):
    """sp = 1/4 (G1 + G1^T + G2) in place of 1/4 (G1 + G1^T + 2 G2) on the pair levels with more than one kept sample"""
    case = cc.cases()[name]
    ref = cc.reference(case)
    worst = []
    for l, (f, c) in enumerate(case.levels):
        if c is None or ref.n[l] < 2:
            continue
        F, C = _rows(case, l)
        us, usp = _level_units(case, l, *gx.xcov_identities(F, C, g2_weight=1.0))
        assert us <= 1.0 and usp > WIDE, (name, l, us, usp)
        worst.append(usp)
    print("\n{}: G1 + G2 exceeds the gate of sp {:.3g} times at the least".format(name, min(worst)))
    assert len(worst) >= 4


@pytest.mark.parametrize("pair", [False, True])
def test_the_mirror_tile_of_an_off_diagonal_block_is_caught(pair):
    """R = 100: block (0, 1) of the 64-wide tiling stored untransposed -- the tile of its mirror (1, 0).  The result stays
    symmetric; only the reference sees it."""
    case = cc.cases()["legendre_100"]
    l = _level_of(case, 4 * 32 + 3 if pair else 4 * 64 + 3, pair)
    s, sp = gx.xcov_identities(*_rows(case, l))
    for v in (s, sp):
        blk = v[0:36, 64:100].copy()                       # the 36 x 36 corner the two blocks of 100 terms share
        v[0:36, 64:100] = blk.T
        v[64:100, 0:36] = blk
        assert np.array_equal(v, v.T)
    us, usp = _level_units(case, l, s, sp)
    print("\nmirrored block, level {}: {:.3g} / {:.3g} times the gates".format(l, us, usp))
    assert us > WIDE and usp > WIDE


@pytest.mark.parametrize("pair", [False, True])
def test_a_term_window_starting_one_term_early_is_caught(pair):
    """R = 100: the second term window starts at term 63 instead of 64 -- every entry with i or j >= 64 is that of the term
    before; symmetric still"""
    case = cc.cases()["legendre_100"]
    l = _level_of(case, 4 * 32 + 3 if pair else 4 * 64 + 3, pair)
    s, sp = gx.xcov_identities(*_rows(case, l))
    idx = np.concatenate([np.arange(64), np.arange(63, 99)])
    us, usp = _level_units(case, l, s[np.ix_(idx, idx)], sp[np.ix_(idx, idx)])
    print("\nwindow from term 63, level {}: {:.3g} / {:.3g} times the gates".format(l, us, usp))
    assert us > WIDE and usp > WIDE


@pytest.mark.parametrize("name", ["legendre_17", "legendre_64"])
def test_the_coarse_row_read_one_sample_late_is_caught(name):
    case = cc.cases()[name]
    B = cc.batches(case.kernel)[0]
    l = _level_of(case, 4 * B + 3, True)
    F, C = _rows(case, l)
    us, usp = _level_units(case, l, *gx.xcov_identities(F[:, :-1], C[:, 1:]))
    print("\n{}: coarse one sample late: {:.3g} / {:.3g} times the gates".format(name, us, usp))
    assert us > WIDE and usp > WIDE


@pytest.mark.parametrize("name,i,j,seen", [("legendre_17", 1, 1, True), ("legendre_17", 16, 16, True), ("legendre_64", 2, 1, False),
                                           ("legendre_64", 63, 63, False), ("monomial_33", 5, 7, True)])
def test_a_linearisation_coefficient_off_in_its_last_ten_bits(name, i, j, seen):
    """The largest coefficient of entry (i, j) of the product table multiplied by 1 + 2^-43, on the largest level without coarse
    values (every extended sum is of the order of n there): 560 / 189 units against a gate of 128 at 17 moments, 1020 against 18
    for monomials (one coefficient per entry) -- seen, asserted.  At 64 moments the gate is 664 units and the flaw 75 / 61: this
    class does not see ten bits of one coefficient (printed, not asserted: a sharper class may); tests/test_linearize.py pins the
    tables to exact rationals instead."""
    case = cc.cases()[name]
    R, K = case.desc.size, 2 * case.desc.size - 1
    l = _level_of(case, 4 * cc.batches(case.kernel)[1] + 3, False)
    table = cc.lib_table(case.desc, 0).copy()
    ext = ax.level_sums(cx.extended(case.desc, K), case.levels, np.float64).s.reshape(case.L, case.M, K)
    key, want, scale = cc.judged(case, "lin", l, "s")
    e = i * R + j
    sound = ax.unit_errors(cx.lin_contract(table, ext)[l, 0], want, scale)[e]
    k = int(np.argmax(table[:, i, j] * np.abs(ext[l, 0])))
    table[k, i, j] *= 1.0 + 2.0 ** -43
    units = float(ax.unit_errors(cx.lin_contract(table, ext)[l, 0], want, scale)[e])
    print("\n{} entry ({}, {}) coefficient {}: {:.3g} units before, {:.3g} after, gate {:.4g}".format(name, i, j, k, float(sound), units, cc.tolerance(key)))
    assert sound <= cc.tolerance(key)
    print("    seen" if units > cc.tolerance(key) else "    NOT seen by this class")
    assert units > cc.tolerance(key) or not seen, (units, cc.tolerance(key))


# ---------------------------------------------------------------------------------------------------------------------------
# the old gates
# ---------------------------------------------------------------------------------------------------------------------------
def test_new_tolerances_in_the_form_of_the_old_gates():
    """The new tolerance of every class rewritten as the old gates were: the means 1e-10 of max(|s|, sqrt(|sp| n)) (direct) and
    1e-12 of sqrt(|sp| n) (linearised), the second moments 1e-10 of |sp| (direct; entries above 1e-3 of the largest) and 1e-11 of
    max(|sp|, 1e-3 max|sp|) (linearised).  Worst entry per class; the classes where the new gate is NOT below the old one are
    listed and pinned."""
    worst, every = {}, {}
    for case in cc.cases().values():
        if case.entry == "diff":
            continue
        ref = cc.reference(case)
        for route in case.routes[:2]:
            for l in range(case.L):
                n = ref.n[l]
                if n < 2:
                    continue
                rms = np.sqrt(np.abs(ref.sp[l]) * n)
                big = np.max(np.abs(ref.sp[l]))
                for q in ("s", "sp"):
                    key, want, scale = cc.judged(case, route, l, q)
                    new = cc.tolerance(key) * ax.U * scale
                    if q == "s":
                        old = (1e-12 * rms) if key[1] == "lin" else 1e-10 * np.maximum(np.abs(want), rms)
                        live = old > 0
                    elif key[1] == "lin":
                        old, live = 1e-11 * np.maximum(np.abs(want), 1e-3 * big), np.ones(want.shape, dtype=bool)
                    else:
                        old, live = 1e-10 * np.abs(want), np.abs(want) > 1e-3 * big
                    if live.any():
                        ratio = (new[live] / old[live]).astype(np.float64)
                        worst[key] = max(worst.get(key, 0.0), float(np.max(ratio)))
                        every.setdefault(key, []).append(ratio)
    print()
    for key in sorted(worst):
        print("{:18s} {:6s} {:4s} {:2s} new gate / old gate, worst entry: {:.3g}, median entry: {:.3g}".format(
            *key, worst[key], float(np.median(np.concatenate(every[key])))))
    above = sorted(k for k, v in worst.items() if v >= 1.0)
    print("not below the old gate:", above)
    assert above == NOT_BELOW_THE_OLD_GATE, above


# log and spline: the budget of one rounding of the logarithm / of the knot variable is part of the unit and was not part of the
# old gates (splines: by the WORST entry, one that only a sample next to a knot reaches and whose value is ~0; the median entry of
# every spline class is below the old gate, printed); TransformedMoments: the old gate of sp is relative to |sp| of the entry, the unit to sum (|T| a)_i^2 (|T| a)_j^2
# the linearised means of 33..64 (pair levels) and 65..128 moments (levels without coarse values): the old gate there was 1e-12
# of sqrt(|sp| n), and the route's own emulation (second term window, connection table) sits 144 / 822 units from the reference
NOT_BELOW_THE_OLD_GATE = sorted(
    [("legendre<=128", "lin", "0", "s"), ("legendre<=64", "lin", "pair", "s")] +
    [("log", r, lv, q) for r, lv, q in (("direct", "0", "s"), ("direct", "0", "sp"), ("direct", "pair", "s"), ("direct", "pair", "sp"),
                                        ("lin", "0", "s"), ("lin", "0", "sp"), ("lin", "pair", "s"))]
    + [("spline{}".format(R), "direct", lv, q) for R in (37, 128) for lv in ("0", "pair") for q in ("s", "sp")]
    + [("spline8", "direct", "pair", "sp")]
    + [(b, "direct", lv, "sp") for b in ("transformed", "transformed>128") for lv in ("0", "pair")])
