"""CPU checks of the extended-precision max-entropy reference (tests/maxent_exact.py): the long-double sums against mpmath at
50 digits, the Gauss-Legendre rule, and the calibration of the plain-fp64 twin against the reference over the case table of
tests/maxent_cases.py.  The calibration table is printed (pytest -s shows it) and pinned by the constants TWIN_UNITS of
tests/maxent_cases.py, from which tests/test_gpu_maxent_exact.py derives the device tolerances."""
import mpmath
import numpy as np
import pytest

from oracle import oracle_np as onp
from tests import maxent_cases as mc
from tests import maxent_exact as mx

LD = np.longdouble


def test_long_double_is_extended_precision():
    """without an 80-bit long double the module proves nothing: a failure, not a skip"""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


@pytest.mark.parametrize("n", [1, 2, 10, 21, 64])
def test_gauss_legendre_ld(n):
    x, w = mx.gauss_legendre_ld(n)
    eps = np.finfo(LD).eps
    assert x.dtype == LD and np.all(np.diff(x) > 0) and np.array_equal(x, -x[::-1]) and np.array_equal(w, w[::-1])
    assert abs(np.sum(w) - 2) <= 4 * n * eps
    assert abs(np.sum(w * x ** (2 * n - 1))) <= 4 * n * eps                       # the highest degree the rule integrates
    assert abs(np.sum(w * x ** (2 * n - 2)) - LD(2) / (2 * n - 1)) <= 4 * n * eps   # and the highest even one
    x64 = np.polynomial.legendre.leggauss(n)[0]
    assert np.max(np.abs(x.astype(np.float64) - x64)) <= 4e-16


# ---------------------------------------------------------------------------------------------------------------------------
# mpmath, 50 digits
# ---------------------------------------------------------------------------------------------------------------------------
def _mp_gauss(n):
    x0 = mx.gauss_legendre_ld(n)[0]
    xs, ws = [], []
    for z in x0:
        z = mpmath.findroot(lambda t: mpmath.legendre(n, t), mpmath.mpf(float(z))) if abs(z) > 0 else mpmath.mpf(0)
        dp = n * (z * mpmath.legendre(n, z) - mpmath.legendre(n - 1, z)) / (z * z - 1)
        xs.append(z)
        ws.append(2 / ((1 - z * z) * dp * dp))
    return xs, ws


def _mp_bspline(j, p, u, knots, span):
    """Cox-de Boor recursion; `span` = the knot span whose polynomial piece is used (a point that the fp64 transform puts ON the
    end of the reference domain may lie 1e-17 beyond it in exact arithmetic: the end pieces extend as polynomials)"""
    if p == 0:
        return mpmath.mpf(1) if j == span else mpmath.mpf(0)
    out = mpmath.mpf(0)
    if knots[j + p] > knots[j]:
        out += (u - knots[j]) / (knots[j + p] - knots[j]) * _mp_bspline(j, p - 1, u, knots, span)
    if knots[j + p + 1] > knots[j + 1]:
        out += (knots[j + p + 1] - u) / (knots[j + p + 1] - knots[j + 1]) * _mp_bspline(j + 1, p - 1, u, knots, span)
    return out


def _mp_basis(desc, x, size):
    """rows of the basis at mpf x from the textbook definitions (mpmath.legendre, powers, cos / sin, recursive Cox-de Boor)"""
    m = mpmath.mpf
    v = mpmath.log(x) if desc.log else x
    t = (v - m(desc.shift)) * m(desc.scale) + m(desc.ref_domain[0])
    n_und = desc.size if desc.matrix is not None else size
    if desc.kind == mx.LEGENDRE:
        und = [mpmath.legendre(i, t) for i in range(n_und)]
    elif desc.kind == mx.MONOMIAL:
        und = [t ** i for i in range(n_und)]
    elif desc.kind == mx.FOURIER:
        und = [m(1)] + [mpmath.cos((i + 1) // 2 * t) if i % 2 else mpmath.sin((i + 1) // 2 * t) for i in range(1, n_und)]
    else:
        ns = desc.size - 3
        knots = [m(min(max(k, 0), ns)) / ns for k in range(-3, ns + 4)]
        u = (t - m(desc.ref_domain[0])) / (m(desc.ref_domain[1]) - m(desc.ref_domain[0]))
        span = min(max(int(mpmath.floor(u * ns)), 0), ns - 1) + 3
        und = [m(1)] + [_mp_bspline(j, 3, u, knots, span) for j in range(1, n_und)]
    if desc.matrix is None:
        return und, [abs(p) for p in und]
    rows = [sum(m(float(desc.matrix[i, k])) * und[k] for k in range(n_und)) for i in range(size)]
    arows = [sum(abs(m(float(desc.matrix[i, k])) * und[k]) for k in range(n_und)) for i in range(size)]
    return rows, arows


def _mp_exponent(phi, aphi, lam, sigma):
    m = mpmath.mpf
    e = -sum(p * m(float(l)) / m(float(s)) for p, l, s in zip(phi, lam, sigma))
    c = 1 + sum(p * abs(m(float(l))) / m(float(s)) for p, l, s in zip(aphi, lam, sigma))
    return mpmath.exp(min(max(e, m(-200)), m(200))), c


def _close(got, want, scale):
    """|got - want| <= 2^-58 scale, got long double, want / scale mpf"""
    hi, lo = float(got), float(got - LD(float(got)))
    return abs(mpmath.mpf(hi) + mpmath.mpf(lo) - want) <= mpmath.mpf(2) ** -58 * scale


@pytest.mark.parametrize("name,R1", [("mix_R9", 5), ("norm12_R7", 7)])
def test_functional_against_mpmath(name, R1):
    """F, g, H, moment0 and their scales on a 4 x 5 rule at perturbed start multipliers: the long-double sums agree with 50-digit
    arithmetic to 2^-58 of the condition scale (2^-5 of the unit the device is judged in)."""
    c = mc.cases()[name]
    assert c.R1 >= R1
    lam, mu, sig = mc.perturbed(c.lam0)[:R1], c.mu[:R1], c.sigma[:R1]
    a, b = c.domain
    ref = mx.functional_ld(c.desc, mu, sig, lam, a, b, 4, 5)
    with mpmath.workdps(50):
        m = mpmath.mpf
        gx, gw = _mp_gauss(5)
        h = (m(b) - m(a)) / 4
        F = sum(m(float(mu[i])) * m(float(lam[i])) / m(float(sig[i])) for i in range(R1))
        Fs = sum(abs(m(float(mu[i])) * m(float(lam[i])) / m(float(sig[i]))) for i in range(R1))
        g = [m(float(mu[i])) / m(float(sig[i])) for i in range(R1)]
        gs = [abs(v) for v in g]
        H = [[m(0)] * R1 for _ in range(R1)]
        Hs = [[m(0)] * R1 for _ in range(R1)]
        m0 = ms = m(0)
        for k in range(4):
            lo = m(a) + k * h
            hi = m(b) if k == 3 else m(a) + (k + 1) * h
            for z, wz in zip(gx, gw):
                x, w = (z + 1) / 2 * (hi - lo) + lo, wz * (hi - lo) / 2
                phi, aphi = _mp_basis(c.desc, x, R1)
                rho, cq = _mp_exponent(phi, aphi, lam, sig)
                m0 += w * rho
                ms += w * rho * cq
                for i in range(R1):
                    si = m(float(sig[i]))
                    g[i] -= w * rho * phi[i] / si
                    gs[i] += w * rho * cq * aphi[i] / si
                    for j in range(R1):
                        sj = m(float(sig[j]))
                        H[i][j] += w * rho * phi[i] * phi[j] / (si * sj)
                        Hs[i][j] += w * rho * cq * aphi[i] * aphi[j] / (si * sj)
        assert _close(ref["moment0"], m0, ms) and _close(ref["F"], F + m0, Fs + ms)
        assert _close(ref["m_scale"], ms, ms) and _close(ref["F_scale"], Fs + ms, Fs + ms)
        for i in range(R1):
            assert _close(ref["g"][i], g[i], gs[i]) and _close(ref["g_scale"][i], gs[i], gs[i]), i
            for j in range(R1):
                assert _close(ref["H"][i, j], H[i][j], Hs[i][j]) and _close(ref["H_scale"][i, j], Hs[i][j], Hs[i][j]), (i, j)


@pytest.mark.parametrize("name", ["monomial_R6", "fourier_R9", "spline_R10", "log_legendre_R8"])
def test_density_against_mpmath(name):
    c = mc.cases()[name]
    lam = mc.perturbed(c.lam0)
    a, b = c.domain
    x = np.concatenate([np.linspace(a, b, 9), [a + (b - a) / 7]])     # 1/7: on a knot of the spline (ns = 7)
    rho, scale, _ = mx.density_ld(c.desc, lam, c.sigma, x)
    with mpmath.workdps(50):
        for k, xv in enumerate(x):
            phi, aphi = _mp_basis(c.desc, mpmath.mpf(float(xv)), c.R1)
            want, cq = _mp_exponent(phi, aphi, lam, c.sigma)
            assert _close(rho[k], want, want * cq) and _close(scale[k], want * cq, want * cq), (name, k)


def test_basis_ld_matches_the_fp64_oracle():
    """values of the oracle to fp64 rounding, NaN positions exactly the oracle's"""
    kinds = {mx.LEGENDRE: onp.LEGENDRE, mx.MONOMIAL: onp.MONOMIAL, mx.FOURIER: onp.FOURIER, mx.SPLINE: onp.SPLINE}
    for name, c in mc.cases().items():
        if c.R1 > 41:
            continue
        d = c.desc
        ob = onp.Basis(kinds[d.kind], d.size, d.domain, d.ref_domain, d.log, True, d.matrix)
        assert ob.scale == d.scale and ob.shift == d.shift
        x = mc.density_points(c.domain, 101)
        want = onp.eval_all(ob, x, c.R1)
        if d.kind == mx.FOURIER:
            want[np.isnan(want[:, 1]), 0] = np.nan              # the oracle keeps the constant column in masked rows
        got, agot = mx.basis_ld(d, x, c.R1)
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        ok = ~np.isnan(want)
        # derivative of P_n is at most n^2 / 2 at the ends; t carries a few fp64 roundings, amplified by |x| / width
        amp = 1 + abs(d.shift) * d.scale
        bound = 1e-15 * amp * (1 + c.desc.size ** 2) * np.maximum(1.0, agot.astype(np.float64))
        assert np.all(np.abs(got.astype(np.float64) - want)[ok] <= bound[ok]), (name, np.max(np.abs(got.astype(np.float64) - want)[ok]))


def test_scales_are_permutation_invariant_and_hessian_is_symmetric():
    c = mc.cases()["norm110_R21"]
    lam = mc.perturbed(c.lam0)
    a, b = c.domain
    ref = mx.functional_ld(c.desc, c.mu, c.sigma, lam, a, b, 7, 21)
    assert np.array_equal(ref["H"], ref["H"].T) and np.array_equal(ref["H_scale"], ref["H_scale"].T)
    # the same sums over permuted nodes
    x, w = mx.composite_rule(a, b, 7, 21)
    perm = np.random.default_rng(5).permutation(len(x))
    phi, aphi = mx.basis_ld(c.desc, x[perm], c.R1)
    ls = lam.astype(LD) / c.sigma.astype(LD)
    _, rho, cq = mx._rho(phi, aphi, ls, LD)
    wrc = w[perm] * rho * cq
    eps = np.finfo(LD).eps
    lin = np.sum(np.abs(c.mu.astype(LD) * ls))
    assert abs(np.sum(wrc) - ref["m_scale"]) <= 32 * eps * ref["m_scale"]
    assert abs(lin + np.sum(wrc) - ref["F_scale"]) <= 32 * eps * ref["F_scale"]
    gs = np.abs(c.mu / c.sigma).astype(LD) + (wrc @ aphi) / c.sigma.astype(LD)
    assert np.all(np.abs(gs - ref["g_scale"]) <= 32 * eps * ref["g_scale"])
    aps = aphi / c.sigma.astype(LD)[None, :]
    Hs = (aps * wrc[:, None]).T @ aps
    assert np.all(np.abs(Hs - ref["H_scale"]) <= 32 * eps * ref["H_scale"])


def test_far_start_needs_backtracking():
    """the far-start case is one where the reference shows that the full Newton step from the start INCREASES F, so a solver
    has to backtrack or regularise before it returns"""
    for c in mc.cases().values():
        if not c.far:
            continue
        a, b = c.domain
        f0 = mx.functional_ld(c.desc, c.mu, c.sigma, c.lam0, a, b, *mc.DEFAULT_QUAD)
        p = -np.linalg.solve(f0["H"].astype(np.float64), f0["g"].astype(np.float64))
        f1 = mx.functional_ld(c.desc, c.mu, c.sigma, c.lam0 + p, a, b, *mc.DEFAULT_QUAD, hess=False)
        print(f"{c.name}: F(lam0) = {float(f0['F']):.6g}, F(lam0 + p) = {float(f1['F']):.6g}")
        assert f1["F"] > f0["F"]


# ---------------------------------------------------------------------------------------------------------------------------
# calibration of the twin
# ---------------------------------------------------------------------------------------------------------------------------
def _twin_row(c, lam, quad):
    a, b = c.domain
    r = mx.functional_ld(c.desc, c.mu, c.sigma, lam, a, b, *quad)
    t = mx.functional_f64(c.desc, c.mu, c.sigma, lam, a, b, *quad)
    mc.assert_clip_band(r["e"])
    return dict(F=mx.units(t["F"], r["F"], r["F_scale"]), g=mx.units(t["g"], r["g"], r["g_scale"]),
                H=mx.units(t["H"], r["H"], r["H_scale"]), m=mx.units(t["moment0"], r["moment0"], r["m_scale"]))


def _density_rows(c, lam):
    x = mc.density_points(c.domain)
    r, rs, e = mx.density_ld(c.desc, lam, c.sigma, x)
    mc.assert_clip_band(e)
    t, _, _ = mx.density(c.desc, lam, c.sigma, x, np.float64)
    lo, hi = mc.integrate_intervals(c.domain)
    worst_i = 0.0
    for deg in mc.INTEGRATE_DEGREES:
        ri, rsc = mx.integrate_ld(c.desc, lam, c.sigma, lo, hi, deg)
        ti, _ = mx.integrate(c.desc, lam, c.sigma, lo, hi, deg, np.float64)
        worst_i = max(worst_i, mx.units(ti, ri, rsc))
    return dict(rho=mx.units(t, r, rs), I=worst_i)


def test_twin_calibration_table():
    """The error of the plain-fp64 twin in units of u * scale, per case and quantity, at: the start, the twin's own Newton
    iterates 1, 3 and 7, its converged multipliers on the default rule and on every other rule of the table, and the perturbed
    multipliers.  Printed, and pinned: the per-class maxima stay within mc.TWIN_UNITS (class 'shifted' = the narrow domain at
    1e3, whose nodes and transform lose log2(|x| / width) = 17 bits in ANY fp64 evaluation; 'regular' = everything else)."""
    worst = {cls: {k: (0.0, None) for k in ("F", "g", "H", "m", "rho", "I")} for cls in ("regular", "shifted")}
    print()
    print(f"{'case':26s} {'at':12s} {'F':>9s} {'g':>9s} {'H':>9s} {'moment0':>9s} {'density':>9s} {'integral':>9s}")
    for name, c in mc.cases().items():
        cls = mc.tolerance_class(c)
        trace = []
        lam = mc.newton_f64(c, mc.DEFAULT_QUAD, trace=trace)
        pts = [("start", c.lam0, mc.DEFAULT_QUAD)]
        pts += [(f"iterate {k}", trace[k], mc.DEFAULT_QUAD) for k in (1, 3, 7) if k < len(trace) - 1]
        pts += [(f"conv {q[0]}x{q[1]}", lam, q) for q in mc.QUADRATURES]
        pts += [("perturbed", mc.perturbed(lam), mc.DEFAULT_QUAD)]
        for tag, l, quad in pts:
            cq = mc.on_rule(c, quad)                  # truncated to R1 = degree where the rule's own P_degree is in the family
            row = _twin_row(cq, l[:cq.R1], quad)
            if tag in ("conv 64x21", "perturbed"):
                row.update(_density_rows(c, l))
            print(f"{name:26s} {tag:12s} " + " ".join(f"{row[k]:9.3g}" if k in row else " " * 9 for k in ("F", "g", "H", "m", "rho", "I")))
            for k, v in row.items():
                if v > worst[cls][k][0]:
                    worst[cls][k] = (v, f"{name} / {tag}")
    print()
    for cls in worst:
        for k, (v, where) in worst[cls].items():
            print(f"max twin error, class {cls:8s} {k:4s}: {v:10.4g} units at {where}   (pinned: {mc.TWIN_UNITS[cls][k]})")
    for cls in worst:
        for k, (v, where) in worst[cls].items():
            assert np.isfinite(v) and v <= mc.TWIN_UNITS[cls][k], (cls, k, v, where)
            # the constants are maxima, not slack: the measured value is not far below what is pinned
            assert v >= 0.5 * mc.TWIN_UNITS[cls][k], (cls, k, v, where)


def test_one_interval_rule_with_its_own_legendre_polynomial_is_degenerate():
    """why mc.on_rule truncates these problems to R1 = degree: with the column of P_degree the twin is not within any sensible
    number of units; without it, it is"""
    c = mc.cases()["mix_R9"]
    assert mc.on_rule(c, (1, 5)).R1 == 5 and mc.on_rule(c, (1, 21)) is c and mc.on_rule(c, (7, 5)) is c
    assert mc.on_rule(c, (1, 5), to_convergence=True).R1 == 5 and mc.on_rule(mc.cases()["monomial_R6"], (1, 5), True) is None
    row = _twin_row(c, c.lam0, (1, 5))
    print("mix_R9 on the 1 x 5 rule, twin:", row)
    assert row["H"] > 1e9
    cut = mc.on_rule(c, (1, 5))
    row = _twin_row(cut, cut.lam0, (1, 5))
    print("mix_R9[:5] on the 1 x 5 rule, twin:", row)
    assert row["H"] <= mc.TWIN_UNITS["regular"]["H"]


def test_give_up_start_admits_no_step():
    """mc.give_up_case: on the reference, the Newton step from the start fails the Armijo test at every step length the solvers
    try (1, 1/2, ... 2^-39), and the Hessian at the rejected trial point is far outside the tolerance of the one at the start"""
    c = mc.give_up_case()
    a, b = c.domain
    f0 = mx.functional_ld(c.desc, c.mu, c.sigma, c.lam0, a, b, *mc.DEFAULT_QUAD)
    mc.assert_clip_band(f0["e"])
    g, H = f0["g"].astype(np.float64), f0["H"].astype(np.float64)
    assert np.all(np.linalg.eigvalsh(H) > 0)
    p = -np.linalg.solve(H, g)
    gp = float(g @ p)
    assert gp < 0
    for k in range(40):
        alpha = 2.0 ** -k
        ft = mx.functional_ld(c.desc, c.mu, c.sigma, c.lam0 + alpha * p, a, b, *mc.DEFAULT_QUAD, hess=False)
        assert ft["F"] > f0["F"] + np.longdouble(1e-4 * alpha * gp) * 100, k          # short of the demand by a factor > 100
    f1 = mx.functional_ld(c.desc, c.mu, c.sigma, c.lam0 + p, a, b, *mc.DEFAULT_QUAD)
    assert mx.units(f1["H"].astype(np.float64), f0["H"], f0["H_scale"]) > 100 * mc.device_tolerance(c, "H")


def test_clip_case_straddles_both_bounds():
    for name in mc.CLIP_CASES:
        c = mc.cases()[name]
        lam = mc.newton_f64(c, mc.DEFAULT_QUAD)
        x = mc.density_points(c.domain)
        lc = mc.clip_multipliers(c, lam)
        rho, _, e = mx.density_ld(c.desc, lc, c.sigma, x)
        mc.assert_clip_band(e)
        fin = np.isfinite(e)
        assert np.any(e[fin] > 200) and np.any(e[fin] < -200) and np.any(np.abs(e[fin]) < 200)
        assert np.all(rho[fin][e[fin] > 200].astype(np.float64) == np.exp(200.0))
        assert np.all(rho[fin][e[fin] < -200].astype(np.float64) == np.exp(-200.0))
