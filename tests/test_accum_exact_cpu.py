"""CPU checks of the extended-precision reference of the accumulated level sums (tests/accum_exact.py): its long-double rows and
complete sums against mpmath at 50 digits, its spline rows against scipy, its masks and counts against the oracle, and the
calibration of the two fp64 twins over the case table of tests/accum_cases.py; a deliberately flawed twin shows what the
tolerances catch.  The calibration table is printed (pytest -s shows it) and pinned by the constants TWIN_UNITS /
EVAL_TWIN_UNITS of tests/accum_cases.py, from which tests/test_gpu_accum_exact.py derives the device tolerances."""
import mpmath
import numpy as np
import pytest

from oracle import oracle_np as onp
from tests import accum_cases as ac
from tests import accum_exact as ax

LD = np.longdouble
_KIND = {ax.LEGENDRE: onp.LEGENDRE, ax.MONOMIAL: onp.MONOMIAL, ax.FOURIER: onp.FOURIER, ax.SPLINE: onp.SPLINE}


def test_long_double_is_extended_precision():
    """without an 80-bit long double the module proves nothing: a failure, not a skip"""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


# ---------------------------------------------------------------------------------------------------------------------------
# mpmath, 50 digits
# ---------------------------------------------------------------------------------------------------------------------------
def _mp(v):
    """exact mpf of a long double (or double)"""
    frac, exp = np.frexp(LD(v))                   # t^51 of the values next to t = 0 lies below the range of a double
    hi = float(frac)
    return mpmath.ldexp(mpmath.mpf(hi) + mpmath.mpf(float(frac - LD(hi))), int(exp))


def _mp_bspline(j, p, u, knots, span):
    if p == 0:
        return mpmath.mpf(1) if j == span else mpmath.mpf(0)
    out = mpmath.mpf(0)
    if knots[j + p] > knots[j]:
        out += (u - knots[j]) / (knots[j + p] - knots[j]) * _mp_bspline(j, p - 1, u, knots, span)
    if knots[j + p + 1] > knots[j + 1]:
        out += (knots[j + p + 1] - u) / (knots[j + p + 1] - knots[j + 1]) * _mp_bspline(j + 1, p - 1, u, knots, span)
    return out


def _mp_t(desc, x):
    """the transformed value the reference is defined on: log=False the fp64 t (exactly), log=True from the raw value"""
    m = mpmath.mpf
    if desc.log:
        return (mpmath.log(m(float(x))) - m(desc.shift)) * m(desc.scale) + m(desc.ref_domain[0])
    return m(float((np.float64(x) - desc.shift) * desc.scale + desc.ref_domain[0]))


def _mp_rows(desc, t):
    """[phi_k(t)], [|phi_k'(t)|] from the textbook definitions in mpf: Bonnet's recurrence in exact rational coefficients (against
    mpmath.legendre for the low degrees), powers, cos / sin, recursive Cox-de Boor"""
    m = mpmath.mpf
    R = desc.size
    if desc.kind == ax.LEGENDRE:
        p = [m(1), t]
        for i in range(2, R):
            p.append(((2 * i - 1) * t * p[i - 1] - (i - 1) * p[i - 2]) / i)
        p = p[:R]
        for i in range(0, min(R, 40), 7):
            assert abs(p[i] - mpmath.legendre(i, t)) < m(10) ** -40
        # P'_k = k (t P_k - P_{k-1}) / (t^2 - 1) away from the ends, k (k + 1) / 2 (+-1)^(k+1) at them
        if t * t == 1:
            dp = [m(k * (k + 1)) / 2 for k in range(R)]
        else:
            dp = [m(0)] + [k * (t * p[k] - p[k - 1]) / (t * t - 1) for k in range(1, R)]
    elif desc.kind == ax.MONOMIAL:
        p = [t ** i for i in range(R)]
        dp = [m(0)] + [i * t ** (i - 1) for i in range(1, R)]
    elif desc.kind == ax.FOURIER:
        p = [m(1)] + [mpmath.cos((i + 1) // 2 * t) if i % 2 else mpmath.sin((i + 1) // 2 * t) for i in range(1, R)]
        dp = [m(0)] * R
    else:
        ns = R - 3
        knots = [m(min(max(k, 0), ns)) / ns for k in range(-3, ns + 4)]
        u = (t - m(desc.ref_domain[0])) / (m(desc.ref_domain[1]) - m(desc.ref_domain[0]))
        span = min(max(int(mpmath.floor(u * ns)), 0), ns - 1) + 3
        p = [m(1)] + [_mp_bspline(j, 3, u, knots, span) if span - 3 <= j <= span else m(0) for j in range(1, R)]
        dp = [m(0)] * R
    return p, [abs(v) for v in dp]


def _row_scale(desc, p):
    """the scale of a row value: |value| for the monomial products (an error relative to the value), 1 otherwise"""
    return [abs(v) for v in p] if desc.kind == ax.MONOMIAL else [mpmath.mpf(1)] * len(p)


ROW_CASES = [ax.Desc(ax.LEGENDRE, 512, ac.DOM), ax.Desc(ax.LEGENDRE, 50, ac.LOG_DOM, log=True), ax.Desc(ax.MONOMIAL, 52, ac.MONO_DOM),
             ax.Desc(ax.FOURIER, 128, ac.DOM), ax.Desc(ax.SPLINE, 128, ac.DOM), ax.Desc(ax.SPLINE, 8, ac.DOM)]


@pytest.mark.parametrize("desc", ROW_CASES, ids=repr)
def test_rows_against_mpmath(desc):
    """every hand-placed value of the case table and seven ordinary ones: the long-double rows agree with 50-digit arithmetic to
    2^-58 of the scale (2^-5 of the unit the device is judged in).  Fourier: up to k t = 64 * 2 pi, the largest argument the
    table has (k t is exact in long double: 53 + 7 bits)."""
    x = np.array([v for pair in ac.edge_pairs(desc) for v in pair] + list(np.linspace(desc.domain[0], desc.domain[1], 9)[1:-1] * 0.97))
    got, keep = ax.eval_rows(desc, x)
    assert keep.sum() >= 20 and (~keep).sum() >= 2
    assert np.all(np.isnan(got[~keep])) and np.all(np.isfinite(got[keep]))
    worst = mpmath.mpf(0)
    with mpmath.workdps(50):
        for i in np.flatnonzero(keep):
            p, _ = _mp_rows(desc, _mp_t(desc, x[i]))
            # log=True: the long-double t itself carries the rounding of logl, far inside the budget E of the sums
            extra = [abs(v) * 2 * desc.scale * abs(np.log(x[i])) for v in _mp_rows(desc, _mp_t(desc, x[i]))[1]] if desc.log else None
            for k, (want, sc) in enumerate(zip(p, _row_scale(desc, p))):
                if extra is not None:
                    sc = sc + extra[k]
                err = abs(_mp(got[i, k]) - want)
                assert err <= mpmath.mpf(2) ** -58 * sc, (desc, x[i], k, float(err / sc))
                if sc > 0:
                    worst = max(worst, err / sc)
    print("{!r}: worst row error 2^{:.1f} of the scale".format(desc, float(mpmath.log(worst, 2)) if worst > 0 else -np.inf))


SUM_CASES = ["legendre_64_63x64x65", "legendre_130_63x64x65", "legendre_512_1", "monomial_33_63x64x65", "fourier_33_63x64x65", "spline_37_63x64x65",
             "log_20_127x129x1", "vector3_17_63x64x65"]


@pytest.mark.parametrize("name", SUM_CASES)
def test_complete_sums_against_mpmath(name):
    """s, sp and their scales S, SP of whole cases, summed in mpf over the samples the reference keeps"""
    case = ac.cases()[name]
    desc, ref = case.desc, ac.reference(case)
    R = desc.size
    with mpmath.workdps(50):
        m = mpmath.mpf
        for l, (f, c) in enumerate(case.levels):
            keep = np.ones(f.shape[1], dtype=bool)
            for side in (f,) if c is None else (f, c):
                for row in side:
                    keep &= ax.transform(desc, row, np.float64)[1]
            assert keep.sum() == ref.n[l]
            for comp in range(case.M):
                s, sp, S, SP = ([m(0)] * R for _ in range(4))
                for i in np.flatnonzero(keep):
                    pf, dpf = _mp_rows(desc, _mp_t(desc, f[comp, i]))
                    wf = 2 * desc.scale * abs(np.log(f[comp, i])) if desc.log else 0
                    if c is None:
                        pc, dpc, wc = [m(0)] * R, [m(0)] * R, 0
                    else:
                        pc, dpc = _mp_rows(desc, _mp_t(desc, c[comp, i]))
                        wc = 2 * desc.scale * abs(np.log(c[comp, i])) if desc.log else 0
                    d = [a - b for a, b in zip(pf, pc)]
                    a = [abs(u) + abs(v) + du * wf + dv * wc for u, v, du, dv in zip(pf, pc, dpf, dpc)]
                    s = [x + y for x, y in zip(s, d)]
                    sp = [x + y * y for x, y in zip(sp, d)]
                    S = [x + y for x, y in zip(S, a)]
                    SP = [x + y * y + 2 * abs(y) * z for x, y, z in zip(SP, d, a)]
                for k in range(R):
                    j = comp * R + k
                    assert abs(_mp(ref.s[l, j]) - s[k]) <= m(2) ** -58 * S[k], (name, l, k)
                    assert abs(_mp(ref.sp[l, j]) - sp[k]) <= m(2) ** -58 * SP[k], (name, l, k)
                    assert abs(_mp(ref.S[l, j]) - S[k]) <= m(2) ** -50 * S[k], (name, l, k)
                    assert abs(_mp(ref.SP[l, j]) - SP[k]) <= m(2) ** -50 * SP[k], (name, l, k)
                    if SP[k] == 0:
                        assert ref.SP[l, j] == 0 and ref.sp[l, j] == 0


def test_covariance_sums_against_mpmath():
    """sum (f_i f_j - c_i c_j) and its scale of one covariance case"""
    case = ac.cases()["cov_5_65x64x1"]
    ref = ac.reference(case)
    R = case.desc.size
    with mpmath.workdps(50):
        m = mpmath.mpf
        for l, (f, c) in enumerate(case.levels):
            s = [[m(0)] * R for _ in range(R)]
            S = [[m(0)] * R for _ in range(R)]
            keep = ax.transform(case.desc, f[0], np.float64)[1] & (True if c is None else ax.transform(case.desc, c[0], np.float64)[1])
            for n in np.flatnonzero(keep):
                pf = _mp_rows(case.desc, _mp_t(case.desc, f[0, n]))[0]
                pc = [m(0)] * R if c is None else _mp_rows(case.desc, _mp_t(case.desc, c[0, n]))[0]
                for i in range(R):
                    for j in range(R):
                        s[i][j] += pf[i] * pf[j] - pc[i] * pc[j]
                        S[i][j] += (abs(pf[i]) + abs(pc[i])) * (abs(pf[j]) + abs(pc[j]))
            for i in range(R):
                for j in range(R):
                    assert abs(_mp(ref.s[l, i * R + j]) - s[i][j]) <= m(2) ** -58 * S[i][j], (l, i, j)
                    assert abs(_mp(ref.S[l, i * R + j]) - S[i][j]) <= m(2) ** -50 * S[i][j], (l, i, j)


# ---------------------------------------------------------------------------------------------------------------------------
# scipy, the oracle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ac.SPLINE_R)
def test_spline_rows_against_scipy(R):
    """the project pins its splines against scipy.interpolate.BSpline: so does the reference (fp64 design matrix)"""
    desc = ax.Desc(ax.SPLINE, R, ac.DOM)
    x = np.concatenate([[v for pair in ac.edge_pairs(desc) for v in pair], np.linspace(-4, 4, 501)])
    got, keep = ax.eval_rows(desc, x)
    ref = onp.eval_all(onp.Basis(onp.SPLINE, R, ac.DOM), x)
    assert np.array_equal(keep, ~np.isnan(ref[:, 1]))
    # scipy takes the knots as fl(k / ns), 2^-53 (relative) off the knots k / ns of the reference: a value moves by |B'| <= 1.5 ns
    # times that
    assert np.max(np.abs(got[keep].astype(np.float64) - ref[keep])) <= (R - 3) * 2.0 ** -52


def test_masks_and_counts_equal_the_oracle():
    """on every case: the keep decision of every value is the oracle's transform, the counts of a level those of its
    estimate_mean (any NaN row drops the sample from all rows)"""
    for case in ac.cases().values():
        ref = ac.reference(case)
        for m, desc in enumerate(case.descs):
            b = onp.Basis(_KIND[desc.kind], desc.size, desc.domain, log=desc.log, safe_eval=desc.safe_eval)
            assert b.scale == desc.scale and b.shift == desc.shift
            levels = ac.component_levels(case, m) if case.entry == "component" else case.levels
            for l, (f, c) in enumerate(levels):
                x = f[:, :, None] if c is None else np.stack([f, c], axis=-1)
                t = onp.transform(b, x)
                for side, raw in enumerate((f,) if c is None else (f, c)):
                    for row in range(raw.shape[0]):
                        assert np.array_equal(ax.transform(desc, raw[row], np.float64)[1], ~np.isnan(t[row, :, side])), case
                _, n_rm = onp.mask_nan_samples(t)
                n_ref, rm_ref = (ref.n[l, m], ref.n_rm[l, m]) if case.entry == "component" else (ref.n[l], ref.n_rm[l])
                assert n_rm == rm_ref and f.shape[1] - n_rm == n_ref, (case, l)
    # and through the oracle's own estimate for a vector quantity with NaNs
    case = ac.cases()["vector3_17_257x1000x5"]
    b = onp.Basis(onp.LEGENDRE, 17, ac.DOM)
    from tests.util import to_chunks
    est = onp.estimate_mean(to_chunks(case.levels), lambda x: onp.moments_rows(b, x))
    ref = ac.reference(case)
    assert np.array_equal(est.n_samples, ref.n) and np.array_equal(est.n_rm_samples, ref.n_rm)
    assert np.all(ref.n_rm > 0) and np.all(ref.n > 0)


def test_the_table_holds_what_it_claims():
    """every level of every case holds the hand-placed values: t = +-1 exactly, a kept value one ulp above the domain, a dropped
    one below, a NaN and a pair with fine == coarse (levels too short for the whole list hold its head)"""
    for case in ac.cases().values():
        for m, desc in enumerate(case.descs):
            for f, c in case.levels:
                pairs = ac.level_pairs(desc, c is not None)
                rows = [m] if case.entry == "component" else range(case.M)
                fv = np.concatenate([f[r] for r in rows])
                for vf, vc in pairs[:f.shape[1]]:
                    assert np.any(fv == vf) or (np.isnan(vf) and np.any(np.isnan(fv))), (case, vf)
                    if c is not None:
                        cv = np.concatenate([c[r] for r in rows])
                        assert np.any(cv == vc) or (np.isnan(vc) and np.any(np.isnan(cv))), (case, vc)
                assert f.shape[1] <= 4099
    d = ax.Desc(ax.LEGENDRE, 8, ac.DOM)
    t, keep, _ = ax.transform(d, np.array([4.0, -4.0, np.nextafter(4.0, 0), np.nextafter(4.0, 9), np.nextafter(-4.0, -9),
                                           np.nextafter(-4.0, 0), np.nextafter(np.nextafter(-4.0, 0), 0), 0.0, -0.0]), np.float64)
    assert list(keep) == [True, True, True, True, False, True, True, True, True]
    assert list(t[:4]) == [1.0, -1.0, 1.0, 1.0] and t[5] == -1 + 2.0 ** -53 and t[6] == -1 + 2.0 ** -52 and t[7] == 0 and t[8] == 0
    x_hi = [v for v, _ in ac.edge_pairs(d)][9]                   # the second double below the upper end: t = 1 - 2^-52
    assert x_hi == 4.0 - 2.0 ** -50 and ax.transform(d, np.array([x_hi]), np.float64)[0][0] == 1 - 2.0 ** -52
    # spline values sit exactly on the knots
    d = ax.Desc(ax.SPLINE, 37, ac.DOM)
    xs = np.array([v for v, _ in ac.edge_pairs(d)])
    t = ax.transform(d, xs, np.float64)[0]
    knots = np.arange(35) / 34
    assert sum(v in knots for v in t) >= 7
    # and no row of a spline level of 63 or more samples is left with a sample at the very end of its support only: every
    # row's scale is at least the value of one spline_fill sample
    for case in ac.cases().values():
        if case.desc.kind == ax.SPLINE:
            ref = ac.reference(case)
            for l, (f, c) in enumerate(case.levels):
                if f.shape[1] >= 63:
                    assert np.min(ref.S[l]) >= 0.01, (case, l, float(np.min(ref.S[l])))


# ---------------------------------------------------------------------------------------------------------------------------
# the twins
# ---------------------------------------------------------------------------------------------------------------------------
def _has_b(desc):
    return desc.kind in (ax.LEGENDRE, ax.FOURIER)


def calibrate():
    """{class: {quantity: [A, B | None]}} and {class: {quantity: (case, variant)}}: the worst units of both twins over every case"""
    table, where = {}, {}
    for case in ac.cases().values():
        ref = ac.reference(case)
        for variant in ("A", "B") if _has_b(case.desc) else ("A",):
            twin = ac.sums_of(case, np.float64, variant)
            assert np.array_equal(twin.n, ref.n) and np.array_equal(twin.n_rm, ref.n_rm)
            for q in ac.quantities(case):
                got, _ = ac.judged(twin, q)
                want, scale = ac.judged(ref, q)
                w, _ = ax.worst(got, want, scale)
                assert np.isfinite(w), (case, q, variant)             # exact zeros where the scale is zero
                row = table.setdefault(case.cls, {}).setdefault(q, [0.0, 0.0 if _has_b(case.desc) else None])
                i = "AB".index(variant)
                if w > row[i]:
                    row[i] = w
                    where.setdefault(case.cls, {})[q, variant] = case.name
    return table, where


def calibrate_eval():
    out = {}
    for name in ac.EVAL_CASES:
        desc, x = ac.eval_desc(name), ac.eval_points(name)
        ref, keep = ax.eval_rows(desc, x)
        scale = np.maximum(np.abs(ref[keep]), 1)
        row = []
        for variant in ("A", "B") if _has_b(desc) else ("A",):
            twin, keep2 = ax.eval_rows(desc, x, np.float64, variant)
            assert np.array_equal(keep, keep2)
            row.append(ax.worst(twin[keep], ref[keep], scale)[0])
        out[name] = row + [None] * (2 - len(row))
    return out


def _two_digits(measured, recorded):
    if recorded is None or measured is None:
        return recorded is None and measured is None
    return abs(measured - recorded) <= 0.01 * recorded


@pytest.fixture(scope="module")
def calibration():
    return calibrate()


def test_twin_calibration_table(calibration):
    """both twins on every case: the worst units per class are the recorded TWIN_UNITS to two digits"""
    table, where = calibration
    print()
    for cls in table:
        for q, (a, b) in table[cls].items():
            print("{:16s} {:6s} twin A {:9.4g} ({})  twin B {}  tolerance {:.4g}".format(
                cls, q, a, where[cls][q, "A"], "{:9.4g} ({})".format(b, where[cls][q, "B"]) if b is not None else "        -",
                max(16.0, 4 * max(a, b or 0.0))))
    assert set(table) == set(ac.TWIN_UNITS)
    for cls in table:
        assert set(table[cls]) == set(ac.TWIN_UNITS[cls]), cls
        for q, (a, b) in table[cls].items():
            ra, rb = ac.TWIN_UNITS[cls][q]
            assert _two_digits(a, ra) and _two_digits(b, rb), (cls, q, a, b, ra, rb)
            assert ac.tolerance(cls, q) == max(16.0, 4.0 * max(ra, rb or 0.0))


def test_eval_twin_calibration_table():
    table = calibrate_eval()
    print()
    for name, (a, b) in table.items():
        print("{:16s} twin A {:9.4g}  twin B {}".format(name, a, "{:9.4g}".format(b) if b is not None else "-"))
    assert set(table) == set(ac.EVAL_TWIN_UNITS)
    for name, (a, b) in table.items():
        ra, rb = ac.EVAL_TWIN_UNITS[name]
        assert _two_digits(a, ra) and _two_digits(b, rb), (name, a, b, ra, rb)
        assert ac.eval_tolerance(name) == 4.0 * max(ra, rb or 0.0)


def test_the_first_gate_is_implied():
    """The gate the accumulation kernels had so far (tests/test_gpu_parity.py, tests/test_gpu_component_moments.py) is
    |a - b| <= 1e-10 max(|b|, rms_level) on the level means and |a - b| <= 1e-10 |b| + 1e-13 on the sums of squares.  On the
    `parity` cases -- every family and size of the table with variances, on the largest size list -- the new tolerance, written
    in that form, stays below it in every entry: a result that passes the new check passes the old one."""
    worst = {}
    u = float(ax.U)
    for case in ac.cases().values():
        if not case.parity:
            continue
        ref = ac.reference(case)
        nn = ref.n[:, None].astype(np.float64)
        s, sp, S, SP = (np.asarray(v, dtype=np.float64) for v in (ref.s, ref.sp, ref.S, ref.SP))
        old = 1e-10 * np.maximum(np.abs(s), np.sqrt(sp * nn))          # max(|mean|, rms) * n
        new = ac.tolerance(case.cls, "s") * u * S
        ok = old > 0
        assert np.all(SP[~ok] == 0)         # d = 0 in every sample: the device test demands s == 0 and sp == 0 exactly there
        w = worst.setdefault(case.cls, [0, 0.0, 0.0])
        w[0] += 1
        w[1] = max(w[1], float(np.max(new[ok] / old[ok])))
        w[2] = max(w[2], float(np.max(ac.tolerance(case.cls, "sp") * u * SP / (1e-10 * sp + 1e-13))))
    print()
    for cls, (n, a, b) in worst.items():
        print("{:16s} {} cases: new tolerance as a fraction of the first gate: means {:.3g}, sums of squares {:.3g}".format(cls, n, a, b))
        assert a < 1 and b < 1, cls
    assert sum(w[0] for w in worst.values()) == len(ac.LEGENDRE_VAR_R) + 9 and len(worst) == 11


def _flawed_sums(desc, levels, i, rel):
    """s, sp of twin B (Bonnet in fp64, coefficients rounded beforehand) with the coefficient a_i off by the relative amount rel"""
    def rows(t):
        v = np.empty((desc.size, t.shape[0]))
        v[0], v[1] = 1, t
        for k in range(2, desc.size):
            a, b = (2.0 * k - 1.0) / k, (k - 1.0) / k
            if k == i:
                a = a * (1 + rel)
            v[k] = a * t * v[k - 1] - b * v[k - 2]
        return v
    s, sp = [], []
    for f, c in levels:
        keep = ax.transform(desc, f[0], np.float64)[1] & (True if c is None else ax.transform(desc, c[0], np.float64)[1])
        d = rows(ax.transform(desc, f[0][keep], np.float64)[0])
        if c is not None:
            d = d - rows(ax.transform(desc, c[0][keep], np.float64)[0])
        s.append(d.sum(axis=1))
        sp.append((d * d).sum(axis=1))
    return np.stack(s), np.stack(sp)


@pytest.mark.parametrize("name", ["legendre_16_257x1000x5", "legendre_48_257x1000x5", "legendre_64_4099x513x2", "legendre_128_257x1000x5",
                                  "legendre_130_257x1000x5", "legendre_512_4099x513x2"])
def test_a_coefficient_wrong_in_its_last_ten_bits_is_caught(name):
    """what the tolerances are for: Bonnet's recurrence with ONE coefficient (a_5) off by 2^-43 -- its last ten bits, a
    relative error of 1.1e-13 that the 1e-10 gate passes 900 times over -- exceeds the class tolerance of s and of sp in every
    size band, by a factor of 3 at least"""
    case = ac.cases()[name]
    ref = ac.reference(case)
    s, sp = _flawed_sums(case.desc, case.levels, 5, 2.0 ** -43)
    sound = ac.sums_of(case, np.float64, "B")
    assert np.array_equal(_flawed_sums(case.desc, case.levels, 5, 0.0)[0], sound.s)        # the local recurrence is twin B
    for q, got in (("s", s), ("sp", sp)):
        want, scale = ac.judged(ref, q)
        assert ax.worst(got, want, scale)[0] > 3 * ac.tolerance(case.cls, q), (name, q)
