"""The case table of the extended-precision max-entropy checks, shared by tests/test_maxent_exact_cpu.py (calibration of the
fp64 twin) and tests/test_gpu_maxent_exact.py (the device).  Plain NumPy data: nothing here touches the device."""
import os

import numpy as np

from tests import maxent_exact as mx

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (n_intervals, gauss_degree): Q = 1344 (default), 5, 21, 35, 147, 4200 -- multiples and non-multiples of 16, 32 and 256
QUADRATURES = ((64, 21), (1, 5), (1, 21), (7, 5), (7, 21), (200, 21))
DEFAULT_QUAD = (64, 21)
# (tol, max_it): converged, and exits on the iteration cap after a line search
STOPPING = ((1e-8, 100), (1e-300, 1), (1e-300, 3), (1e-300, 7))
MIXTURE_R1 = (1, 2, 9, 16, 17, 26, 64, 65, 127, 128)
G6_KEYS = tuple(f"{name}_R{R}" for name in ("norm12", "norm110", "lognorm") for R in (7, 21, 41))


def on_rule(case, quad, to_convergence=False):
    """The problem a case poses on a quadrature: the case itself, a truncated copy, or None.  Decided by the shapes alone.

    1. A plain Legendre family that contains P_degree, on a ONE-interval rule, is truncated to R1 = degree (P_0 .. P_{degree-1};
       the basis object keeps its size, so this is also an R1 < basis-size problem).  The nodes of that rule are the zeros
       of P_degree, so column `degree` of the basis matrix is zero in exact arithmetic and pure rounding in any finite
       precision: the first-order condition scale sum w rho c |phi_i| |phi_j| of that entry is itself at the rounding level --
       the fp64 twin sits 1e15 units from the reference there (test_maxent_exact_cpu.py shows it), so the unit measures
       nothing.  Only that column and the ones above it are left out.  Orthogonalised bases (|L| . |phi|) and the other
       families have no such column and stay whole.
    2. None for a solve run TO CONVERGENCE on a rule with fewer nodes than moments (Q < R1).  The Hessian
       Phi^T diag(w rho) Phi then has rank <= Q < R1, the functional has no minimiser, and the iteration runs off along the
       null space: the cooperative solver returned multipliers of 1e18 for the Monomial case on the 1 x 5 rule, where the
       exponent is a difference of terms of 1e18 and u c_q = 100 -- no fp64 evaluation, the twin included, has a correct digit
       there.  The same problems are solved on every such rule under an iteration cap of 3 steps, where the multipliers stay
       moderate, so every kernel still sees R1 > Q."""
    n_int, deg = quad
    d = case.desc
    if n_int == 1 and d.kind == mx.LEGENDRE and d.matrix is None and case.R1 > deg:
        case = Case(f"{case.name}[:{deg}]", d, case.mu[:deg], case.sigma[:deg], case.lam0[:deg], case.group, case.far)
    if to_convergence and n_int * deg < case.R1:
        return None
    return case


def on_rule_cases(quad, to_convergence=False):
    out = [on_rule(c, quad, to_convergence) for c in cases().values()]
    return [c for c in out if c is not None]


class Case:
    def __init__(self, name, desc, mu, sigma, lam0, group, far=False):
        self.name, self.desc, self.group, self.far = name, desc, group, far
        self.mu = np.ascontiguousarray(mu, dtype=np.float64)
        self.sigma = np.ascontiguousarray(sigma, dtype=np.float64)
        self.lam0 = np.ascontiguousarray(lam0, dtype=np.float64)
        self.R1 = len(self.lam0)
        self.domain = desc.domain

    def __repr__(self):
        return self.name


def uniform_start(R1, dom):
    lam0 = np.zeros(R1)
    lam0[0] = -np.log(1.0 / (dom[1] - dom[0]))
    return lam0


def _gauss_pdf(x, m, s):
    return np.exp(-0.5 * ((x - m) / s) ** 2) / (s * np.sqrt(2 * np.pi))


def mixture_pdf(x):
    return 0.6 * _gauss_pdf(x, 0.5, 1.0) + 0.4 * _gauss_pdf(x, 2.5, 0.7)


def moments_of(desc, pdf, size, normalise=False):
    """moments of a density on a 256 x 21 composite rule in plain fp64 (input data of a case, not a reference)"""
    x, w = mx.composite_rule(desc.domain[0], desc.domain[1], 256, 21, np.float64)
    phi, _ = mx.basis(desc, x, size, np.float64)
    d = pdf(x) * w
    if normalise:
        d = d / np.sum(d)
    return d @ phi


_CASES = None


def cases():
    """name -> Case.  Groups: 'g6' (orthogonalised Legendre bases of the G6 fixtures), 'mixture' (plain Legendre on a
    two-Gaussian mixture), 'other' (one each: Monomial, Fourier, Spline, log, sigma spread, R1 < basis size) and 'shifted'
    (the narrow domain [1e3, 1e3 + 1e-2])."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = {}
    g5 = np.load(os.path.join(GOLDEN, "G5_ortho.npz"))
    g6 = np.load(os.path.join(GOLDEN, "G6_maxent.npz"))
    for key in G6_KEYS:
        R = int(key.rsplit("_R", 1)[1])
        dom = tuple(float(v) for v in g5[key + "_domain"])
        desc = mx.Desc(mx.LEGENDRE, R, dom, matrix=g6[key + "_L"])
        data = g6[key + "_moment_data"]
        out[key] = Case(key, desc, data[:, 0], np.sqrt(data[:, 1]), uniform_start(desc.out_size, dom), "g6")
    dom = (-4.0, 6.0)
    for R in MIXTURE_R1:
        desc = mx.Desc(mx.LEGENDRE, R, dom)
        out[f"mix_R{R}"] = Case(f"mix_R{R}", desc, moments_of(desc, mixture_pdf, R), np.ones(R), uniform_start(R, dom), "mixture")
    desc = mx.Desc(mx.LEGENDRE, 26, dom)
    out["mix_R26_far"] = Case("mix_R26_far", desc, moments_of(desc, mixture_pdf, 26), np.ones(26),
                              uniform_start(26, dom) + 3.0 * np.sin(np.arange(26)), "mixture", far=True)
    # Monomial on ref_domain (-1, 1): on the default (0, 1) the Hessian of this target has condition 1e9 and the Newton
    # iteration of ANY fp64 solver stalls at a gradient norm of 5e-9 -- next to the tolerance 1e-8, so whether the case counts
    # as converged would be decided by rounding.  (-1, 1) converges to 1e-14 and still instantiates the Monomial kernels.
    for name, kind, R, ref in (("monomial_R6", mx.MONOMIAL, 6, (-1.0, 1.0)), ("fourier_R9", mx.FOURIER, 9, None),
                               ("spline_R10", mx.SPLINE, 10, None)):
        desc = mx.Desc(kind, R, dom, ref_domain=ref)
        out[name] = Case(name, desc, moments_of(desc, mixture_pdf, R, True), np.ones(R), uniform_start(R, dom), "other")
    # log = True Legendre basis on a log-normal target
    ldom = (0.2, 12.0)
    desc = mx.Desc(mx.LEGENDRE, 8, ldom, log=True)
    lognormal = lambda x: np.exp(-0.5 * ((np.log(x) - 0.5) / 0.5) ** 2) / (x * 0.5 * np.sqrt(2 * np.pi))
    out["log_legendre_R8"] = Case("log_legendre_R8", desc, moments_of(desc, lognormal, 8, True), np.ones(8), uniform_start(8, ldom), "other")
    # standard errors spread over 1e-3 .. 1, as construct_density produces them from moment variances
    desc = mx.Desc(mx.LEGENDRE, 12, dom)
    sig = np.logspace(0, -3, 12)
    out["sigma_spread_R12"] = Case("sigma_spread_R12", desc, moments_of(desc, mixture_pdf, 12, True), sig, uniform_start(12, dom), "other")
    # R1 smaller than the basis: the first 9 functions of an orthogonalised G6 basis
    key = "norm12_R21"
    gdom = tuple(float(v) for v in g5[key + "_domain"])
    desc = mx.Desc(mx.LEGENDRE, 21, gdom, matrix=g6[key + "_L"])
    data = g6[key + "_moment_data"]
    out["partial_R9_of_norm12_R21"] = Case("partial_R9_of_norm12_R21", desc, data[:9, 0], np.sqrt(data[:9, 1]), uniform_start(9, gdom), "other")
    # shifted narrow domain
    sdom = (1e3, 1e3 + 1e-2)
    desc = mx.Desc(mx.LEGENDRE, 6, sdom)
    narrow = lambda x: _gauss_pdf(x, 1e3 + 4e-3, 2e-3)
    out["shifted_R6"] = Case("shifted_R6", desc, moments_of(desc, narrow, 6, True), np.ones(6), uniform_start(6, sdom), "shifted")
    _CASES = out
    return out


def perturbed(lam):
    """multipliers away from any normalised density: lambda + 0.3 sin(k)"""
    return np.asarray(lam, dtype=np.float64) + 0.3 * np.sin(np.arange(len(lam)))


def newton_f64(case, quad, tol=1e-9, max_it=100, trace=None):
    """Damped Newton on the fp64 twin (Armijo backtracking, diagonal shift when the step is no descent direction): supplies
    the CPU calibration with converged multipliers and intermediate iterates.  Not a reference for anything."""
    lam = case.lam0.copy()
    a, b = case.domain
    tau = 0.0
    for it in range(max_it + 1):
        f = mx.functional_f64(case.desc, case.mu, case.sigma, lam, a, b, *quad)
        if trace is not None:
            trace.append(lam.copy())
        if np.linalg.norm(f["g"]) < tol or it == max_it:
            break
        try:
            p = -np.linalg.solve(f["H"] + tau * np.eye(case.R1), f["g"])
        except np.linalg.LinAlgError:
            p = None
        gp = None if p is None else f["g"] @ p
        alpha, ok = 1.0, False
        if gp is not None and gp < 0:
            for _ in range(40):
                ft = mx.functional_f64(case.desc, case.mu, case.sigma, lam + alpha * p, a, b, *quad, hess=False)
                if ft["F"] <= f["F"] + 1e-4 * alpha * gp:
                    ok = True
                    break
                alpha *= 0.5
        if not ok:
            tau = 1e-10 * (1 + abs(f["F"])) if tau == 0.0 else tau * 100
            if tau > 1e20:
                break
            continue
        lam = lam + alpha * p
    return lam


def density_points(dom, n_grid=1001):
    """the points of the density checks: a grid over the domain (both end points included), nextafter outside each end, far
    outside, NaN, +-inf, -0.0"""
    a, b = dom
    grid = np.linspace(a, b, n_grid)
    grid[0], grid[-1] = a, b
    extra = [np.nextafter(a, -np.inf), np.nextafter(b, np.inf), a - 10 * (b - a), b + 10 * (b - a), np.nan, np.inf, -np.inf, -0.0]
    return np.concatenate([grid, extra])


def cdf_partition(dom, values):
    """(lo, hi) of the intervals SimpleDistribution.cdf integrates for `values`"""
    lo, hi, last = [], [], dom[0]
    for v in values:
        if dom[0] < v < dom[1]:
            lo.append(last)
            hi.append(v)
            last = v
    return np.array(lo), np.array(hi)


INTEGRATE_DEGREES = (1, 2, 10, 21, 64)


def integrate_intervals(dom):
    """intervals of the mlmc_density_integrate checks: the whole domain, a zero-width interval, reversed limits, then the cdf
    partitions of a 127-point and a 131-point grid (125 + 129 intervals); 257 in all, so prefixes of 1, 256 and 257 exist"""
    a, b = dom
    lo1, hi1 = cdf_partition(dom, np.linspace(a, b, 127))
    lo2, hi2 = cdf_partition(dom, np.linspace(a, b, 131))
    mid = a + 0.375 * (b - a)
    lo = np.concatenate([[a, mid, hi1[3]], lo1, lo2])
    hi = np.concatenate([[b, mid, lo1[3]], hi1, hi2])
    assert len(lo) == 257
    return lo, hi


CLIP_CASES = ("mix_R9", "norm12_R21", "fourier_R9")


def clip_multipliers(case, lam):
    """multipliers scaled so that the exponents over the density points span 1200, and shifted in lambda_0 so that they are
    centred on 0: the exponent exceeds +200 at some points and falls below -200 at others"""
    x = density_points(case.domain)
    _, _, e = mx.density_ld(case.desc, lam, case.sigma, x)
    e = e[np.isfinite(e)]
    lc = float(1200 / (np.max(e) - np.min(e))) * np.asarray(lam, dtype=np.float64)
    _, _, e = mx.density_ld(case.desc, lc, case.sigma, x)
    e = e[np.isfinite(e)]
    phi0 = float(mx.basis_ld(case.desc, [0.5 * (case.domain[0] + case.domain[1])], 1)[0][0, 0])      # the constant function
    lc[0] += float(0.5 * (np.min(e) + np.max(e))) * case.sigma[0] / phi0
    return lc


def assert_clip_band(e):
    """no reference exponent within 1e-9 of +-200: the clip decision cannot differ between precisions"""
    e = np.asarray(e)
    e = e[np.isfinite(e)]
    assert not np.any(np.abs(np.abs(e) - 200) <= 1e-9), e[np.abs(np.abs(e) - 200) <= 1e-9]


def tolerance_class(case):
    return "shifted" if case.group == "shifted" else "regular"


# Worst error of the plain-fp64 twin against the long-double reference, in units of u * scale, over the calibration of
# tests/test_maxent_exact_cpu.py::test_twin_calibration_table (which asserts them).  Measured 2026-10-16.
TWIN_UNITS = {
    # F, m: norm12_R41 at perturbed multipliers (27.23 / 27.24); g: the same (41.73); H: mix_R127 at the start (121.7);
    # rho: norm110_R41 perturbed (160.1); I: norm12_R21 perturbed (244.2)
    "regular": dict(F=28.0, g=42.0, H=122.0, m=28.0, rho=161.0, I=245.0),
    # shifted_R6: F, g, H, m on the 1 x 5 rule (truncated to R1 = 5: 7433 / 3.177e4 / 1.287e5 / 1.33e4); rho, I perturbed
    # (1.983 / 1.092e5).  The nodes x = 1e3 + ... and t = (x - shift) * scale lose log2(1e3 / 1e-2) = 17 bits in ANY fp64
    # evaluation, and the device's errors equal the twin's to three digits: what this class measures is that rounding of the
    # nodes.  It constrains the kernels themselves only at about 1e-11 relative (H, integrals), not at the few units of the
    # regular class.
    "shifted": dict(F=7440.0, g=3.18e4, H=1.29e5, m=1.34e4, rho=2.0, I=1.1e5),
}
_DEVICE_KEY = dict(F="F", g="g", H="H", moment0="m", density="rho", integral="I")


def device_tolerance(case, quantity):
    """4 x the twin's worst error with a floor of 16 units.  The kernels sum in another order, evaluate the Legendre rows by
    their own recurrence and use the device exp (<= 1 ulp against the C library's): each a factor of order one on an error of
    a few units.  The solver's gradient and integral sums are compensated, so they should sit BELOW the twin; a kernel that
    needs more than 4 x the uncompensated twin has a defect."""
    return max(16.0, 4.0 * TWIN_UNITS[tolerance_class(case)][_DEVICE_KEY[quantity]])


def give_up_case(quad=DEFAULT_QUAD):
    """A start from which NO step length of the line search can be accepted, so a solver must give up and return the start.

    Plain Legendre R1 = 2 on the mixture moments, exponent e(t) = -lambda_0 + K t with K = 60000: the nodes with e > 200 (a
    third of the domain) are clipped to exp(200) and carry all of g and H, so the Newton direction is the constant function
    (p = (1, 0) to 1e-6) and lowers every exponent by alpha.  The clipped nodes do not move F at all; the only node that does
    is the one just under the clip, placed at e = 192, which carries exp(-8) / 450 = 7e-7 of the mass -- far less than the
    1e-4 |g.p| the Armijo test demands at any step length.  At lambda + p that node's density is smaller by 1 - 1/e: a Hessian
    taken at the rejected trial point differs from the one at the returned multipliers by 1e5 units of its scale."""
    base = cases()["mix_R2"]
    x, _ = mx.composite_rule(base.domain[0], base.domain[1], quad[0], quad[1], np.float64)
    t = (x - base.desc.shift) * base.desc.scale + base.desc.ref_domain[0]
    m = int(np.argmin(np.abs(t - 0.3)))
    K = 60000.0
    lam0 = np.array([K * t[m] - 192.0, -K])
    return Case("give_up_R2", base.desc, base.mu, base.sigma, lam0, "mixture")
