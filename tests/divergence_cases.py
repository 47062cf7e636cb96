"""Pair table, extended-precision reference and fp64 twin of the divergences between max-entropy densities, shared by
tests/test_divergence_cpu.py (calibration of the twin) and tests/test_gpu_divergences.py (the device).  Plain NumPy: nothing here
touches the device.

The definition (include/mlmc_hip.h, mlmc_density_divergences_batch): on [lo, hi] with the fp64 cell edges e_j = lo + j h of
tests/quantile_cases.edges and on every cell the Gauss-Legendre nodes t and weights w, with the clipped exponents e_p, e_q of the
prior and the posterior, rho = exp(e), d = e_q - e_p, x = expm1(d), y = expm1(d / 2), the six columns are the sums of
    KL  w rho_p (x - d)     L2SQ  w rho_p^2 x^2     TV  w rho_p |x| / 2     H2  w rho_p y^2 / 2     MASS_P  w rho_p     MASS_Q  w rho_q.
x^2 is inf where it exceeds the fp64 range (the definition states the product in fp64); a node where either density is NaN makes
all six NaN.  Every value is a finite sum, so `pair_sums(..., np.longdouble)` evaluates it in 80-bit long double;
`pair_sums(..., np.float64)` is the twin that calibrates the tolerance and is never compared with the device.

Condition scales, in the convention of maxent_exact (sums of the absolute values of the terms; c = 1 + sum |phi lambda| / sigma is
the rounding of an exponent in units of u, so d carries c_p + c_q and rho_p carries c_p relative):
    KL    sum |w| rho_p   [|x| + |d| + (x - d) c_p + |x| (c_p + c_q)]                     (d/dd (x - d) = x)
    L2SQ  sum |w| rho_p^2 [x^2 (2 + 2 c_p) + 2 |x| (1 + x) (c_p + c_q)]                   (d/dd x^2 = 2 x (1 + x))
    TV    sum |w| rho_p   [|x| (1 + c_p) + (1 + x) (c_p + c_q)] / 2
    H2    sum |w| rho_p   [y^2 (2 + c_p) + |y| (1 + y) (c_p + c_q)] / 2                   (d/dd y^2 = y (1 + y))
    MASS  sum |w| rho c."""
import numpy as np

from tests import maxent_cases as mc
from tests import maxent_exact as mx
from tests import quantile_cases as qc

LD = np.longdouble
U = 2.0 ** -53
KL, L2SQ, TV, H2, MASS_P, MASS_Q = range(6)
COLUMNS = ("kl", "l2sq", "tv", "h2", "mass_p", "mass_q")
F64_MAX = np.finfo(np.float64).max

SELF_CASES = ("mix_R9", "norm12_R21", "fourier_R9", "shifted_R6")
CROSS = (("mix_R9", "converged", "fourier_R9", "converged"), ("monomial_R6", "converged", "spline_R10", "converged"),
         ("sigma_spread_R12", "converged", "mix_R9", "perturbed"))
G6_CROSS = (("norm12_R21", "norm110_R21"), ("lognorm_R7", "norm12_R7"))


X2_OVERFLOW_D = 0.5 * float(np.log(F64_MAX))                 # expm1(d)^2 leaves the fp64 range above d = 354.891...


def assert_overflow_band(d):
    """no reference d within 1e-6 of the overflow of x^2: the decision cannot differ between precisions"""
    d = np.asarray(d, dtype=np.float64)
    assert not np.any(np.abs(d - X2_OVERFLOW_D) <= 1e-6), d[np.abs(d - X2_OVERFLOW_D) <= 1e-6]


def _gauss(deg, dtype):
    return mx.gauss_legendre_ld(deg) if dtype is LD else np.polynomial.legendre.leggauss(deg)


def node_values(case, lam, t, dtype):
    """(clipped exponent, rho, c) of one density at the nodes t; NaN outside the basis' domain or for NaN multipliers"""
    rho, rc, e = mx.density(case.desc, lam, case.sigma, t, dtype)
    with np.errstate(all="ignore"):
        return np.minimum(np.maximum(e, dtype(-200)), dtype(200)), rho, rc / rho


def pair_sums(prior, posterior, interval, quad, dtype=LD, exponents=None):
    """(values [6], scales [6]) of the pair prior = (case, lam), posterior = (case, lam) on `interval` = (lo, hi) and the rule
    `quad`, in `dtype`; all six values NaN when a node of either density is.  exponents (a list, optional) receives the unclipped
    exponents of both densities at the nodes and d."""
    n = quad[0] if quad[0] > 0 else 64
    deg = quad[1] if quad[1] > 0 else 21
    e = qc.edges(interval, n)
    gx, gw = _gauss(deg, dtype)
    lo, hi = e[:-1].astype(dtype), e[1:].astype(dtype)
    half, mid = (hi - lo) / 2, (hi + lo) / 2                                     # the node arithmetic of the definition
    t = (half[:, None] * gx[None, :] + mid[:, None]).ravel()                     # (density_integral): the twin rounds as the rule does
    aw = np.abs(gw[None, :] * half[:, None]).ravel()                             # the weights are positive
    ep, rp, cp = node_values(prior[0], prior[1], t, dtype)
    eq, rq, cq = node_values(posterior[0], posterior[1], t, dtype)
    if exponents is not None:
        exponents.extend([mx.density(prior[0].desc, prior[1], prior[0].sigma, t, dtype)[2],
                          mx.density(posterior[0].desc, posterior[1], posterior[0].sigma, t, dtype)[2], eq - ep])
    with np.errstate(all="ignore"):
        d = eq - ep
        x, y = np.expm1(d), np.expm1(d / 2)
        xx = np.where(x * x > F64_MAX, dtype(np.inf), x * x)
        cd = cp + cq
        vals = [np.sum(aw * rp * (x - d)), np.sum(aw * (rp * rp) * xx), np.sum(aw * rp * np.abs(x)) / 2, np.sum(aw * rp * (y * y)) / 2,
                np.sum(aw * rp), np.sum(aw * rq)]
        scales = [np.sum(aw * rp * (np.abs(x) + np.abs(d) + (x - d) * cp + np.abs(x) * cd)),
                  np.sum(aw * (rp * rp) * (xx * (2 + 2 * cp) + 2 * np.abs(x) * (1 + x) * cd)),
                  np.sum(aw * rp * (np.abs(x) * (1 + cp) + (1 + x) * cd)) / 2,
                  np.sum(aw * rp * (y * y * (2 + cp) + np.abs(y) * (1 + y) * cd)) / 2,
                  np.sum(aw * rp * cp), np.sum(aw * rq * cq)]
    vals, scales = np.array(vals, dtype=dtype), np.array(scales, dtype=dtype)
    if np.any(np.isnan(rp)) or np.any(np.isnan(rq)):
        vals[:] = np.nan
    return vals, scales


class Pair:
    """one pair of the table: prior / posterior = (case, lam), the interval, the rule and the tolerance class"""

    def __init__(self, tag, prior, posterior, quad, interval=None):
        self.prior, self.posterior, self.quad = prior, posterior, quad
        (a0, b0), (a1, b1) = prior[0].domain, posterior[0].domain
        self.interval = (max(a0, a1), min(b0, b1)) if interval is None else interval
        assert self.interval[0] < self.interval[1], tag
        self.cls = "shifted" if "shifted" in (mc.tolerance_class(prior[0]), mc.tolerance_class(posterior[0])) else "regular"
        self.tag = f"{tag} {quad[0]}x{quad[1]}"
        self.same = prior[0] is posterior[0] and np.array_equal(prior[1], posterior[1])

    def reference(self, dtype=LD):
        return pair_sums(self.prior, self.posterior, self.interval, self.quad, dtype)


def pairs(converged=None):
    """The pair table on qc.RULES at the multipliers `converged(case, quad)` gives (default: mc.newton_f64): every case against its
    mc.perturbed self; converged multipliers scaled by 1 + 1e-6 and 1 + 1e-2 (the small-d regime of bootstrap replicates); four
    cases against themselves; three cross-family pairs on the shared domain (-4, 6); two G6 pairs with different domains on
    their intersection.  log_legendre_R8 and shifted_R6 (its own tolerance class) are among the cases."""
    converged = (lambda case, quad: mc.newton_f64(case, quad)) if converged is None else converged
    cases = mc.cases()
    out = []
    for quad in qc.RULES:
        lam = {name: np.asarray(converged(case, quad), dtype=np.float64) for name, case in cases.items()}
        at = {"converged": lambda n: lam[n], "perturbed": lambda n: mc.perturbed(lam[n])}
        for name, case in cases.items():
            out.append(Pair(f"{name} converged / perturbed", (case, lam[name]), (case, mc.perturbed(lam[name])), quad))
            for eps in (1e-6, 1e-2):
                out.append(Pair(f"{name} converged / scaled 1+{eps:g}", (case, lam[name]), (case, lam[name] * (1 + eps)), quad))
        for name in SELF_CASES:
            out.append(Pair(f"{name} / itself", (cases[name], lam[name]), (cases[name], lam[name]), quad))
        for p, kp, q, kq in CROSS:
            assert cases[p].domain == cases[q].domain == (-4.0, 6.0)
            out.append(Pair(f"{p} {kp} / {q} {kq}", (cases[p], at[kp](p)), (cases[q], at[kq](q)), quad))
        for p, q in G6_CROSS:
            assert cases[p].domain != cases[q].domain
            out.append(Pair(f"{p} / {q} on the intersection", (cases[p], lam[p]), (cases[q], lam[q]), quad))
    return out


def units(got, ref, scale):
    """per column |got - ref| / (2^-53 scale); 0 where both are NaN or the same infinity, inf where only one is finite"""
    got, out = np.asarray(got).astype(LD), np.zeros(6)
    for c in range(6):
        if np.isfinite(ref[c]) and np.isfinite(got[c]):
            err = abs(got[c] - ref[c])
            out[c] = 0.0 if err == 0 else float(err / (LD(U) * scale[c]))
        elif not ((np.isnan(ref[c]) and np.isnan(got[c])) or ref[c] == got[c]):
            out[c] = np.inf
    return out


# Worst error of the fp64 twin (pair_sums(..., np.float64)) against the long-double reference over `pairs()`, any column, in units
# of 2^-53 scale; asserted by tests/test_divergence_cpu.py::test_twin_calibration.  Measured on the CPU 2026-10-19.
TWIN_UNITS_D = {
    # norm12_R41 converged / perturbed on 64 x 21, L2SQ: 40.62 (its MASS_Q on 200 x 21 33.36, KL / TV / H2 there 29.72 / 29.72 /
    # 29.45).  Every pair of converged multipliers with their scaled copies stays below 1 unit in the first four columns: the
    # |d| term of the KL scale holds at small d.
    "regular": 40.7,
    # shifted_R6 converged / perturbed on 64 x 21, MASS_Q: 228.09 (MASS_P 227.49 in every pair of the case; KL 42.16, L2SQ 77.25,
    # TV 74.59, H2 47.21).  This is the fp64 rounding of the nodes x = 1e3 + ... of the definition (mid = (hi + lo) / 2 is rounded at
    # the spacing of 1e3 and moves all nodes of a cell together), as in mc.TWIN_UNITS: with nodes formed as lo + (g + 1) / 2 (hi - lo)
    # the same twin stays at 22.4 units, and any evaluation of the definition's nodes in fp64 sits where this one does.
    "shifted": 228.5,
}


def divergence_tolerance(cls):
    """4 x the twin's worst error, at least 16 units (the convention of mc.device_tolerance): the margin covers the device's exp
    and expm1, the kernels' own Legendre recurrence and the fp64 rounding of the nodes"""
    return max(16.0, 4.0 * TWIN_UNITS_D[cls])
