"""Extended-precision reference and fp64 twin of the tail means (expected shortfall) of the max-entropy densities, shared by
tests/test_tail_means_cpu.py (calibration of the twin) and tests/test_gpu_tail_means.py (the device).  Plain NumPy: nothing here
touches the device.

The definition (include/mlmc_hip.h, mlmc_density_tail_means_batch): with the fp64 cell edges e_j, the cell integrals C_j, their
prefix P and T = P_n of tests/quantile_cases.py, and on the same nodes t_k and weights w_k
    A_j = sum_k w_k (t_k - a) rho(t_k),  B_j = sum_k w_k (b - t_k) rho(t_k),
    V_0 = 0, V_{j+1} = V_j + A_j;  S_n = W_n = 0, S_j = S_{j+1} + C_j, W_j = W_{j+1} + B_j,
for x in cell j (the largest j < n with e_j <= x)
    m_lo = P_j + I(e_j, x)          lower(x) = a + (V_j + A(e_j, x)) / m_lo
    m_hi = S_{j+1} + I(x, e_{j+1})  upper(x) = b - (W_{j+1} + B(x, e_{j+1})) / m_hi
and a tail without mass returns x.  Every quantity is a finite sum, so `TailTable(..., np.longdouble)` evaluates it in 80-bit long
double; `TailTable(..., np.float64)` is the twin that calibrates the tolerance and is never compared with the device."""
import numpy as np

from tests import maxent_cases as mc
from tests import maxent_exact as mx
from tests import quantile_cases as qc

LD = np.longdouble
U = 2.0 ** -53

# qc.GRID[::4] and the four extreme probabilities of qc.GRID: 54 points
GRID = np.unique(np.concatenate([qc.GRID[::4], qc.GRID[:2], qc.GRID[-2:]]))


def _gauss(deg, dtype):
    return mx.gauss_legendre_ld(deg) if dtype is LD else np.polynomial.legendre.leggauss(deg)


class TailTable:
    """P, S, V, W of one problem in `dtype`, the tail means at given points and their first-order condition scales in the
    convention of maxent_exact (sums of the absolute values of the terms, each weighted with c = 1 + sum |phi lambda| / sigma):
        scale_lower = (SV(x) + (v / m) SP(x)) / m + v / m + |lower|,   v = V_j + A(e_j, x), m = m_lo(x),
    SP / SV the prefix plus partial sum of sum |w| rho c / sum |w| (t - a) rho c; scale_upper the same from the right."""

    def __init__(self, case, lam, quad, dtype=LD):
        self.case, self.lam, self.dtype = case, np.asarray(lam, dtype=np.float64), dtype
        self.n = quad[0] if quad[0] > 0 else 64
        self.deg = quad[1] if quad[1] > 0 else 21
        self.e = qc.edges(case.domain, self.n)
        self.a, self.b = dtype(self.e[0]), dtype(self.e[-1])
        C, sC, A, sA, B, sB = self.sums(self.e[:-1], self.e[1:])
        zero = np.zeros(1, dtype=dtype)
        fwd = lambda v: np.concatenate([zero, np.cumsum(v)])
        bwd = lambda v: np.concatenate([np.cumsum(v[::-1])[::-1], zero])
        self.P, self.SP, self.V, self.SV = fwd(C), fwd(sC), fwd(A), fwd(sA)
        self.S, self.SS, self.W, self.SW = bwd(C), bwd(sC), bwd(B), bwd(sB)
        self.T = self.P[-1]

    def sums(self, lo, hi):
        """per interval [lo_i, hi_i]: the rule's sums of rho, (t - a) rho, (b - t) rho, each followed by its scale"""
        dtype = self.dtype
        gx, gw = _gauss(self.deg, dtype)
        lo = np.atleast_1d(np.asarray(lo, dtype=np.float64)).astype(dtype)
        hi = np.atleast_1d(np.asarray(hi, dtype=np.float64)).astype(dtype)
        t = (gx[None, :] + 1) / 2 * (hi - lo)[:, None] + lo[:, None]
        w = gw[None, :] * (hi - lo)[:, None] / 2
        rho, rc, _ = mx.density(self.case.desc, self.lam, self.case.sigma, t.ravel(), dtype)
        rho, rc, aw = rho.reshape(t.shape), rc.reshape(t.shape), np.abs(w)
        da, db = t - self.a, self.b - t
        with np.errstate(all="ignore"):
            return (np.sum(w * rho, axis=1), np.sum(aw * rc, axis=1), np.sum(w * da * rho, axis=1), np.sum(aw * np.abs(da) * rc, axis=1),
                    np.sum(w * db * rho, axis=1), np.sum(aw * np.abs(db) * rc, axis=1))

    def mean(self):
        """(a + V_n / T, its scale)"""
        r = self.V[-1] / self.T
        m = self.a + r
        return m, (self.SV[-1] + r * self.SP[-1]) / self.T + r + abs(m)

    def tails(self, x):
        """(lower, upper, scale_lower, scale_upper) at the fp64 points x in [a, b]; NaN for NaN"""
        dtype = self.dtype
        x = np.atleast_1d(np.asarray(x, dtype=np.float64))
        lower, upper = np.full(x.shape, np.nan, dtype=dtype), np.full(x.shape, np.nan, dtype=dtype)
        sl, su = np.ones(x.shape, dtype=dtype), np.ones(x.shape, dtype=dtype)
        ok = ~np.isnan(x)
        if not ok.any():
            return lower, upper, sl, su
        xo = x[ok]
        j = np.clip(np.searchsorted(self.e, xo, side="right") - 1, 0, self.n - 1)
        I0, s0, A0, sA0, _, _ = self.sums(self.e[j], xo)
        I1, s1, _, _, B1, sB1 = self.sums(xo, self.e[j + 1])
        xd = xo.astype(dtype)
        with np.errstate(all="ignore"):
            m, v = self.P[j] + I0, self.V[j] + A0
            r = v / m
            lw = np.where(m == 0, xd, self.a + r)
            scl = np.where(m == 0, np.abs(xd), ((self.SV[j] + sA0) + r * (self.SP[j] + s0)) / m + r + np.abs(lw))
            m, v = self.S[j + 1] + I1, self.W[j + 1] + B1
            r = v / m
            up = np.where(m == 0, xd, self.b - r)
            scu = np.where(m == 0, np.abs(xd), ((self.SW[j + 1] + sB1) + r * (self.SS[j + 1] + s1)) / m + r + np.abs(up))
        lower[ok], upper[ok], sl[ok], su[ok] = lw, up, scl, scu
        return lower, upper, sl, su


def tail_units(ref, x, lower, upper):
    """(units of the lower values, units of the upper values) against the reference table at the points x, per point, in units
    of 2^-53 scale; a value that is not finite where the reference is gives inf"""
    rl, ru, sl, su = ref.tails(x)
    out = []
    for got, want, sc in ((lower, rl, sl), (upper, ru, su)):
        got = np.atleast_1d(np.asarray(got)).astype(LD)
        with np.errstate(all="ignore"):
            u = np.abs(got - want) / (LD(U) * sc)
        u = np.where(np.isnan(want) & np.isnan(got), 0, u)
        out.append(np.where(np.isfinite(u), u, np.inf).astype(np.float64))
    return out[0], out[1]


# Worst error of the fp64 twin (TailTable(..., np.float64).tails at x = qc.twin_quantiles(..., GRID)) against the long-double
# reference at the same x, in units of 2^-53 scale, over qc.used_problems at fp64 Newton multipliers (mc.newton_f64); asserted by
# tests/test_tail_means_cpu.py::test_twin_calibration.  Measured on the CPU 2026-10-18.
TWIN_UNITS_T = {
    # norm12_R41 at perturbed multipliers on the 200 x 21 rule, lower tail at p = 0.41018: 31.78 (next: its upper tail 28.26,
    # norm12_R21 perturbed 200 x 21 upper 11.22, norm110_R21 perturbed 200 x 21 upper 9.19; every converged problem stays
    # below 1.8 units).  The same definition on the full qc.GRID gave 46.1 at the same problem and tail.
    "regular": 32.0,
    # shifted_R6 converged on 64 x 21, upper tail at p = 1: 0.512.  The anchors a and b take the cancellation of the domain
    # [1e3, 1e3 + 1e-2] out of the sums, so this class needs no more than the floor of 16 units.
    "shifted": 0.52,
}


def tail_tolerance(case):
    """4 x the twin's worst error, at least 16 units (the convention of mc.device_tolerance): the margin covers another
    summation order, the device exp and the kernels' own Legendre recurrence"""
    return max(16.0, 4.0 * TWIN_UNITS_T[mc.tolerance_class(case)])
