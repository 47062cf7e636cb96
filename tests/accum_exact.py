"""Extended-precision reference of the accumulated level sums -- TEST INFRASTRUCTURE, plain NumPy.

For a moments object (family, size, domain, log, safe_eval) and the raw fine / coarse values of one level,

    s_k = sum_n d_k(n),   sp_k = sum_n d_k(n)^2,   d_k = phi_k(f) - phi_k(c)   (level 0: d_k = phi_k(f)),

over the samples the reference keeps (quantity_estimate.mask_nan_samples: a NaN in any row of fine or coarse drops the sample
from all rows), evaluated in 80-bit np.longdouble (eps = 2^-63).  Next to every sum comes its first-order condition scale

    S_k = sum (|phi_k(f)| + |phi_k(c)|),      SP_k = sum (d^2 + 2 |d| (|phi_k(f)| + |phi_k(c)|)),

and an error is reported in UNITS of u * scale, u = 2^-53.  Where a scale is exactly zero the value must be exactly zero.

The transform t = (x - shift) * scale + ref0 is part of the contract in fp64 (two roundings, keep decision bit-identical to
NumPy's), so for log=False the reference starts from that fp64 t and everything after it is long double.  For log=True the
device's log may differ from NumPy's in the last bit: t is taken in long double from the raw value and every value adds the
first-order term |phi_k'(t)| * scale * 2^-52 * |log x| (the move of phi_k under one ulp of the logarithm) to the error budget --
in units of u that is E_k = 2 |phi_k'(t)| scale |log x|, added to S_k, and 2 |d| (E_k(f) + E_k(c)) to SP_k.

Every routine takes the working dtype: np.longdouble gives the reference, np.float64 a *twin* (calibration only,
tests/test_accum_exact_cpu.py; no device result is ever compared with a twin):

    twin A  the reference's own operation order (legvander, polyvander, cos / sin(k t)) in plain fp64;
    twin B  the same mathematics with per-step coefficients rounded beforehand, from the textbook: Bonnet's recurrence
            P_i = a_i t P_{i-1} - b_i P_{i-2} with a_i = fl((2i-1)/i), b_i = fl((i-1)/i), and for Fourier the angle-addition
            recurrence from cos t, sin t.  Monomial and Spline have only twin A.

Nothing here imports the package, the device, or the oracle.
"""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53

LEGENDRE, MONOMIAL, FOURIER, SPLINE = "legendre", "monomial", "fourier", "spline"
_DEFAULT_REF = {LEGENDRE: (-1.0, 1.0), MONOMIAL: (0.0, 1.0), FOURIER: (0.0, 2 * np.pi), SPLINE: (0.0, 1.0)}


class Desc:
    """Plain description of a moments object; shift / scale are the fp64 values the package computes (moments.py)."""

    def __init__(self, kind, size, domain, ref_domain=None, log=False, safe_eval=True):
        self.kind = kind
        self.size = int(size)
        self.domain = (float(domain[0]), float(domain[1]))
        self.ref_domain = tuple(float(v) for v in (_DEFAULT_REF[kind] if ref_domain is None else ref_domain))
        self.log = bool(log)
        self.safe_eval = bool(safe_eval)
        lo, hi = (np.log(self.domain[0]), np.log(self.domain[1])) if log else self.domain
        width = max(hi - lo, 1e-15)
        self.scale = float((self.ref_domain[1] - self.ref_domain[0]) / width)
        self.shift = float(lo)

    def __repr__(self):
        return "{}({}, {}{}{})".format(self.kind, self.size, self.domain, ", log" if self.log else "",
                                       "" if self.safe_eval else ", safe_eval=False")


# ---------------------------------------------------------------------------------------------------------------------------
# transform
# ---------------------------------------------------------------------------------------------------------------------------
def transform(desc, x, dtype=LD):
    """-> t (dtype), keep (bool), logw (dtype).  keep is the fp64 decision of the reference's arithmetic (NaN dropped, outside
    [ref0, ref1] dropped with safe_eval).  log=False: t is the fp64 t, widened.  log=True: the long-double reference takes t
    from the raw value in long double, the fp64 twin keeps NumPy's fp64 t; logw = 2 * scale * |log x| (0 without log) is the
    weight of |phi'| in the condition scale.  t of dropped values is 0."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        v64 = np.log(x) if desc.log else x
        t64 = (v64 - desc.shift) * desc.scale + desc.ref_domain[0]
        keep = ~np.isnan(t64)
        if desc.safe_eval:
            keep &= ~((t64 < desc.ref_domain[0]) | (t64 > desc.ref_domain[1]))
        if desc.log and dtype is LD:
            t = (np.log(x.astype(LD)) - LD(desc.shift)) * LD(desc.scale) + LD(desc.ref_domain[0])
        else:
            t = t64.astype(dtype)
        logw = (2 * dtype(desc.scale) * np.abs(v64).astype(dtype)) if desc.log else np.zeros(x.shape, dtype=dtype)
    t = np.where(keep, t, dtype(0))
    logw = np.where(keep, logw, dtype(0))
    return t, keep, logw


# ---------------------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------------------
def rows(desc, t, dtype=LD, variant="A"):
    """phi [size, n] of the family at transformed t [n] (finite), in `dtype`; variant "A" / "B": see the module docstring
    (the long-double reference is variant "A")."""
    t = np.asarray(t, dtype=dtype)
    n, size = t.shape[0], desc.size
    v = np.empty((size, n), dtype=dtype)
    v[0] = 1
    if desc.kind == LEGENDRE:
        if size > 1:
            v[1] = t
        if variant == "A":                              # numpy.polynomial.legendre.legvander
            for i in range(2, size):
                v[i] = (v[i - 1] * t * (2 * i - 1) - v[i - 2] * (i - 1)) / i
        else:                                           # Bonnet with coefficients rounded beforehand
            for i in range(2, size):
                a, b = dtype((2.0 * i - 1.0) / i), dtype((i - 1.0) / i)
                v[i] = a * t * v[i - 1] - b * v[i - 2]
    elif desc.kind == MONOMIAL:
        for i in range(1, size):
            v[i] = v[i - 1] * t
    elif desc.kind == FOURIER:
        if variant == "A":
            for i in range(1, size):
                k = (i + 1) // 2
                v[i] = np.cos(k * t) if i % 2 else np.sin(k * t)
        else:                                           # angle addition from cos t, sin t
            c1, s1 = np.cos(t), np.sin(t)
            c, s = c1.copy(), s1.copy()
            for i in range(1, size):
                k = (i + 1) // 2
                if i % 2 and k > 1:
                    c, s = c * c1 - s * s1, s * c1 + c * s1
                v[i] = c if i % 2 else s
    elif desc.kind == SPLINE:
        # Cox-de Boor on the clamped uniform knots k / ns, in the variable v = u ns with the integer knots k (0 / 0 = 0).  With
        # u an fp64 value and ns < 2^11 the product and every difference v - k are EXACT in long double; with knots rounded to
        # k / ns a value near the end of its support, ~ (u - k / ns)^3, would carry the rounding of the knot at full weight.
        ns = size - 3
        knots = np.clip(np.arange(-3, ns + 4), 0, ns).astype(dtype)
        u = (t - dtype(desc.ref_domain[0])) / (dtype(desc.ref_domain[1]) - dtype(desc.ref_domain[0]))
        u = u * dtype(ns)
        nk = len(knots)
        span = np.clip(np.floor(u).astype(np.int64), 0, ns - 1) + 3
        N = np.zeros((nk - 1, n), dtype=dtype)
        N[span, np.arange(n)] = 1
        for p in range(1, 4):
            M = np.zeros((nk - 1 - p, n), dtype=dtype)
            for j in range(nk - 1 - p):
                d1, d2 = knots[j + p] - knots[j], knots[j + p + 1] - knots[j + 1]
                if d1 > 0:
                    M[j] += (u - knots[j]) / d1 * N[j]
                if d2 > 0:
                    M[j] += (knots[j + p + 1] - u) / d2 * N[j + 1]
            N = M
        v[1:] = N[1:size]
    else:
        raise ValueError(desc.kind)
    return v


def abs_derivative(desc, t, phi):
    """|phi_k'(t)| [size, n] in long double (needed for log=True only).  Legendre: P'_k = P'_{k-2} + (2k-1) P_{k-1}, no division
    by 1 - t^2; Monomial: k t^(k-1); Fourier: k |sin|, k |cos| from the rows themselves."""
    size = desc.size
    dv = np.zeros_like(phi)
    if desc.kind == LEGENDRE:
        for k in range(1, size):
            dv[k] = (dv[k - 2] if k >= 2 else 0) + (2 * k - 1) * phi[k - 1]
    elif desc.kind == MONOMIAL:
        for k in range(1, size):
            dv[k] = k * phi[k - 1]
    elif desc.kind == FOURIER:
        for i in range(1, size):
            k = (i + 1) // 2
            other = i + 1 if i % 2 else i - 1
            dv[i] = k * (phi[other] if other < size else np.sqrt(np.maximum(0, 1 - phi[i] * phi[i])))
    else:
        raise ValueError("log=True is not calibrated for " + desc.kind)
    return np.abs(dv)


def eval_rows(desc, x, dtype=LD, variant="A"):
    """phi [n, size] at raw values x, NaN in the rows of dropped values; keep [n]"""
    t, keep, _ = transform(desc, np.ravel(x), dtype)
    out = np.full((t.shape[0], desc.size), np.nan, dtype=dtype)
    if keep.any():
        out[keep] = rows(desc, t[keep], dtype, variant).T
    return out, keep


# ---------------------------------------------------------------------------------------------------------------------------
# level sums
# ---------------------------------------------------------------------------------------------------------------------------
class Sums:
    """n, n_rm [L]; s, sp and their scales S, SP [L, M * R] (row m * R + r) in the working dtype; phi = per level the kept
    (fine [M, R, n], coarse [M, R, n] | None) rows when asked for."""


def _side(desc, x, keep, dtype, variant):
    """rows [M, R, n_keep] and the log budget E [M, R, n_keep] of one side"""
    M = x.shape[0]
    phi = np.empty((M, desc.size, int(keep.sum())), dtype=dtype)
    E = np.zeros_like(phi)
    for m in range(M):
        t, _, logw = transform(desc, x[m][keep], dtype)
        phi[m] = rows(desc, t, dtype, variant)
        if desc.log:
            if dtype is LD:
                E[m] = abs_derivative(desc, t, phi[m]) * logw[None, :]
    return phi, E


def level_sums(desc, levels, dtype=LD, variant="A", keep_rows=False):
    """levels: list of (fine [M, n], coarse [M, n] | None) raw values -> Sums.  The condition scales of a twin are those of its
    own rows without the log budget (take the reference's)."""
    L = len(levels)
    f0 = np.atleast_2d(levels[0][0])
    K = f0.shape[0] * desc.size
    out = Sums()
    out.n, out.n_rm = np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64)
    out.s, out.sp, out.S, out.SP = (np.zeros((L, K), dtype=dtype) for _ in range(4))
    out.phi = []
    for l, (f, c) in enumerate(levels):
        f = np.atleast_2d(np.asarray(f, dtype=np.float64))
        c = None if c is None else np.atleast_2d(np.asarray(c, dtype=np.float64))
        keep = np.ones(f.shape[1], dtype=bool)
        for side in (f,) if c is None else (f, c):
            for m in range(side.shape[0]):
                keep &= transform(desc, side[m], np.float64)[1]
        out.n[l], out.n_rm[l] = keep.sum(), (~keep).sum()
        pf, Ef = _side(desc, f, keep, dtype, variant)
        if c is None:
            d, a, E, pc = pf, np.abs(pf), Ef, None
        else:
            pc, Ec = _side(desc, c, keep, dtype, variant)
            d, a, E = pf - pc, np.abs(pf) + np.abs(pc), Ef + Ec
        out.s[l] = np.sum(d, axis=-1).reshape(K)
        out.sp[l] = np.sum(d * d, axis=-1).reshape(K)
        out.S[l] = np.sum(a + E, axis=-1).reshape(K)
        out.SP[l] = np.sum(d * d + 2 * np.abs(d) * (a + E), axis=-1).reshape(K)
        out.phi.append((pf, pc) if keep_rows else None)
    return out


def cov_sums(phi):
    """Covariance means from the kept rows of level_sums(..., keep_rows=True) of a scalar quantity: per level
    s_ij = sum (f_i f_j - c_i c_j) and the scale sum (|f_i| + |c_i|)(|f_j| + |c_j|), [L, R * R] (row i * R + j), in the dtype of
    the rows.  The scale bounds the absolute terms of this form and of (d_i s_j + s_i d_j) / 2 alike."""
    s, S = [], []
    for pf, pc in phi:
        F = pf[0]
        if pc is None:
            s.append(F @ F.T)
            A = np.abs(F)
        else:
            Cm = pc[0]
            s.append(F @ F.T - Cm @ Cm.T)
            A = np.abs(F) + np.abs(Cm)
        S.append(A @ A.T)
    R = s[0].shape[0]
    return np.stack(s).reshape(len(s), R * R), np.stack(S).reshape(len(S), R * R)


# ---------------------------------------------------------------------------------------------------------------------------
# errors in units of u * scale
# ---------------------------------------------------------------------------------------------------------------------------
def unit_errors(got, ref, scale):
    """|got - ref| / (u scale) elementwise in long double.  An entry whose scale is exactly zero must be exactly zero (the
    reference is): 0 if so, else inf.  A non-finite `got` gives inf."""
    got = np.asarray(got).astype(LD)
    ref = np.asarray(ref).astype(LD)
    scale = np.broadcast_to(np.asarray(scale).astype(LD), ref.shape)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got - ref)
    with np.errstate(all="ignore"):
        q = np.where(err == 0, LD(0), err / (U * scale))
    q = np.where(scale == 0, np.where(got == 0, LD(0), LD(np.inf)), q)
    return np.where(np.isfinite(got), q, LD(np.inf))


def worst(got, ref, scale):
    """(worst units, flat index of the entry) of unit_errors"""
    q = unit_errors(got, ref, scale)
    i = int(np.argmax(q))
    return float(q.ravel()[i]), i
