"""Test bases, extended-precision reference and fp64 twin of the expectations under a max-entropy density, shared by
tests/test_density_moments_cpu.py (calibration of the twin) and tests/test_gpu_density_moments.py (the device).  Plain NumPy: nothing
here touches the device.

The definition (include/mlmc_hip.h, mlmc_density_moments_batch): on the fp64 cell edges e_j of tests/quantile_cases.edges and on
every cell the Gauss-Legendre nodes t = half g + mid and weights w half, with rho = exp(e), e the clipped exponent of the density,
and psi_k the functions of a test basis of the caller's choice,
    moment k  sum w rho psi_k(t)        mass  sum w rho        entropy  sum w rho (-e).
Every value is a finite sum, so `moment_sums(..., np.longdouble)` evaluates it in 80-bit long double; `moment_sums(..., np.float64)` is
the twin that calibrates the tolerance and is never compared with the device.

Condition scales, in the convention of maxent_exact (c = 1 + sum |phi lambda| / sigma is the rounding of an exponent in units of u, so
rho carries c relative):
    moment k  (sum |w| rho c) B_k,  B_k the sup-norm bound of psi_k on its reference domain: 1 for Legendre, Fourier and spline
              functions, max |ref|^k for monomials, |L| . B for a basis with a matrix L
    entropy   sum |w| rho (|e| + |1 - e| c)                                              (d/de of -e exp(e) is -(1 + e) exp(e))
    mass      sum |w| rho c.
The moment scale does NOT weight with |psi_k(t)|: at the nodes of a 1 x 5 rule P_5 vanishes, sum |w| rho c |P_5| is itself at the
rounding level and covers nothing of the rounding of the node (the fp64 twin sits 2e15 such "units" off there)."""
import numpy as np

from tests import maxent_cases as mc
from tests import maxent_exact as mx
from tests import quantile_cases as qc

LD = np.longdouble
U = 2.0 ** -53

# 64 x 21 and 200 x 21: the rules of the other density checks; 1 x 5: one partly filled tile; 7 x 5: a partial last tile; 3 x 64 and
# 5 x 33: one cell per wave, without and with idle lanes
RULES = ((64, 21), (200, 21), (1, 5), (7, 5), (3, 64), (5, 33))
LEGENDRE300_CASES = ("mix_R9", "norm12_R21", "fourier_R9")           # more columns than threads of a workgroup


def _gauss(deg, dtype):
    return mx.gauss_legendre_ld(deg) if dtype is LD else np.polynomial.legendre.leggauss(deg)


def bases_of(case):
    """name -> (Desc, K) of the test bases of a case: its own basis (a matrix basis for the g6 cases), Legendre 8, a Monomial 5 whose
    reference domain has 0 inside (the centred moments of `summaries`), Fourier 9, spline 10, on a positive domain a log Legendre
    6, and Legendre 300 for three regular cases"""
    dom = case.domain
    out = {"own": (case.desc, case.R1),
           "legendre8": (mx.Desc(mx.LEGENDRE, 8, dom), 8),
           "monomial5c": (mx.Desc(mx.MONOMIAL, 5, dom, ref_domain=(-0.375, 0.625)), 5),
           "fourier9": (mx.Desc(mx.FOURIER, 9, dom), 9),
           "spline10": (mx.Desc(mx.SPLINE, 10, dom), 10)}
    if dom[0] > 0:
        out["loglegendre6"] = (mx.Desc(mx.LEGENDRE, 6, dom, log=True), 6)
    if case.name in LEGENDRE300_CASES:
        out["legendre300"] = (mx.Desc(mx.LEGENDRE, 300, dom), 300)
    return out


def rules_and_bases(case):
    """(quad, base name) of a case's checks: the shifted class on qc.RULES only, with test bases of at most 9 terms"""
    bases = bases_of(case)
    if mc.tolerance_class(case) == "shifted":
        return [(quad, name) for quad in qc.RULES for name, (_, K) in bases.items() if K <= 9]
    return [(quad, name) for quad in RULES for name in bases]


def sup_bounds(desc, K):
    """B_k, k < K: the sup-norm bound of the functions of a basis on its reference domain"""
    und = desc.size if desc.matrix is not None else K
    if desc.kind == mx.MONOMIAL:
        B = max(abs(desc.ref_domain[0]), abs(desc.ref_domain[1])) ** np.arange(und, dtype=np.float64)
    else:
        B = np.ones(und)
    return B if desc.matrix is None else np.abs(desc.matrix[:K]) @ B


_NODE_CACHE = {}


def _nodes(case, lam, quad, dtype):
    """(t, |w|, rho, clipped exponent, c) at the nodes of the definition in `dtype`"""
    key = (case.name, np.asarray(lam, dtype=np.float64).tobytes(), quad, dtype)
    if key not in _NODE_CACHE:
        if len(_NODE_CACHE) > 8:
            _NODE_CACHE.clear()
        n = quad[0] if quad[0] > 0 else 64
        deg = quad[1] if quad[1] > 0 else 21
        e = qc.edges(case.domain, n)
        gx, gw = _gauss(deg, dtype)
        lo, hi = e[:-1].astype(dtype), e[1:].astype(dtype)
        half, mid = (hi - lo) / 2, (hi + lo) / 2                                 # the node arithmetic of the definition
        t = (half[:, None] * gx[None, :] + mid[:, None]).ravel()
        aw = np.abs(gw[None, :] * half[:, None]).ravel()
        rho, rc, ex = mx.density(case.desc, lam, case.sigma, t, dtype)
        with np.errstate(all="ignore"):
            _NODE_CACHE[key] = (t, aw, rho, np.minimum(np.maximum(ex, dtype(-200)), dtype(200)), rc / rho, ex)
    return _NODE_CACHE[key]


def moment_sums(case, lam, test_desc, K, quad, dtype=LD, exponents=None):
    """(values, scales) of the problem (case, lam) with the test basis (test_desc, K) on the rule `quad`, in `dtype`: each a dict
    with "moments" [K], "mass" and "entropy".  All values are NaN when the density is NaN at a node (or the multipliers are), the
    moments alone when the test basis masks a node.  exponents (a list, optional) receives the unclipped exponents."""
    t, aw, rho, e, c, ex = _nodes(case, lam, quad, dtype)
    if exponents is not None:
        exponents.append(ex)
    psi, _ = mx.basis(test_desc, t, K, dtype)
    with np.errstate(all="ignore"):
        wr = aw * rho
        wrc = np.sum(wr * c)
        vals = dict(moments=wr @ psi, mass=np.sum(wr), entropy=np.sum(wr * -e))
        scales = dict(moments=wrc * sup_bounds(test_desc, K).astype(dtype), mass=wrc,
                      entropy=np.sum(wr * (np.abs(e) + np.abs(1 - e) * c)))
    if np.any(np.isnan(rho)):
        vals = dict(moments=np.full(K, np.nan, dtype=dtype), mass=dtype(np.nan), entropy=dtype(np.nan))
    return vals, scales


def units(got, ref, scale):
    """|got - ref| / (2^-53 scale) per entry (scalars or arrays); 0 where both are NaN, inf where only one is finite"""
    got, ref = np.atleast_1d(np.asarray(got)).astype(LD), np.atleast_1d(np.asarray(ref)).astype(LD)
    scale = np.broadcast_to(np.atleast_1d(np.asarray(scale)).astype(LD), ref.shape)
    out = np.zeros(ref.shape)
    for i in range(ref.size):
        if np.isfinite(ref[i]) and np.isfinite(got[i]):
            err = abs(got[i] - ref[i])
            out[i] = 0.0 if err == 0 else float(err / (LD(U) * scale[i]))
        elif not ((np.isnan(ref[i]) and np.isnan(got[i])) or ref[i] == got[i]):
            out[i] = np.inf
    return out


def worst_units(got, ref, scale):
    """{"moments", "mass", "entropy"} -> the worst unit error of the column(s)"""
    return {key: float(np.max(units(got[key], ref[key], scale[key]))) for key in ("moments", "mass", "entropy")}


def twin_table(converged=None):
    """worst error of the fp64 twin against the long-double reference per (class, multipliers, column) with the place it occurs,
    over every case at the multipliers `converged(case)` gives (default: mc.newton_f64 on the 64 x 21 rule) and at
    mc.perturbed(...) of them"""
    converged = (lambda case: mc.newton_f64(case, mc.DEFAULT_QUAD)) if converged is None else converged
    worst = {}
    for case in mc.cases().values():
        lam0 = np.asarray(converged(case), dtype=np.float64)
        for kind, lam in (("converged", lam0), ("perturbed", mc.perturbed(lam0))):
            for quad, name in rules_and_bases(case):
                desc, K = bases_of(case)[name]
                ref, scale = moment_sums(case, lam, desc, K, quad, LD)
                twin, _ = moment_sums(case, lam, desc, K, quad, np.float64)
                for col, v in worst_units(twin, ref, scale).items():
                    key = (mc.tolerance_class(case), kind, col)
                    if v > worst.get(key, (-1.0, None))[0]:
                        worst[key] = (v, f"{case.name} {kind} {name} {quad[0]}x{quad[1]}")
    return worst


# Worst error of the fp64 twin (moment_sums(..., np.float64)) against the long-double reference over twin_table(), in units of
# 2^-53 scale, per tolerance class and kind of multipliers; asserted by tests/test_density_moments_cpu.py::test_twin_calibration.
# Measured on the CPU 2026-10-19 with the nodes of the definition (half g + mid).
TWIN_UNITS_M = {
    # converged: mix_R1 legendre8 on 200 x 21 (moments 4.31; monomial_R6 fourier9 on 5 x 33 4.25), lognorm_R7 own on 1 x 5 (mass
    # 1.09), log_legendre_R8 loglegendre6 on 1 x 5 (entropy 0.52): every rule stays below 4.4 units.
    # perturbed: norm110_R21 on the 3 x 64 rule (moments 156.98 with fourier9, mass 156.99, entropy 209.57 with spline10).  Three
    # cells do not resolve that density: the fp64 rounding of the nodes of the definition moves rho itself.  On the other rules
    # the perturbed problems stay below 96 units (norm12_R21 legendre300 on 5 x 33), on 64 x 21 and 200 x 21 below 43.
    ("regular", "converged"): dict(moments=4.4, mass=1.1, entropy=0.6),
    ("regular", "perturbed"): dict(moments=157.0, mass=157.0, entropy=209.6),
    # shifted_R6 (qc.RULES only, test bases of at most 9 terms): fourier9 on 64 x 21 at converged multipliers (moments 6459.9;
    # on 200 x 21 1373.0 with loglegendre6), mass 228.09 and entropy 217.96 on 64 x 21.  The fp64 rounding of nodes near 1e3 on a
    # domain of width 1e-2, as in dc.TWIN_UNITS_D; a test basis multiplies it with its own slope (cos 4t: 4 x 2 pi / 1e-2 per unit).
    ("shifted", "converged"): dict(moments=6460.0, mass=228.1, entropy=218.0),
    ("shifted", "perturbed"): dict(moments=6460.0, mass=228.1, entropy=218.0),
}


def moment_tolerance(cls, column, kind="converged"):
    """4 x the twin's worst error, at least 16 units (the convention of mc.device_tolerance): the margin covers the device's exp,
    its own recurrences for the density and the test basis and the fp64 rounding of the nodes"""
    return max(16.0, 4.0 * TWIN_UNITS_M[(cls, kind)][column])
