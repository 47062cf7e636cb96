"""Extended-precision reference of the max-entropy functional -- TEST INFRASTRUCTURE, plain NumPy.

For given (basis, mu, sigma, lambda, [a, b], n_intervals, degree) the functional of include/mlmc_hip.h,

    F(lambda) = sum_i mu_i lambda_i / sigma_i + sum_q w_q rho_q,   rho_q = exp(clip(-sum_i phi_i(x_q) lambda_i / sigma_i, +-200)),
    g_i       = mu_i / sigma_i - sum_q w_q rho_q phi_i(x_q) / sigma_i,
    H_ij      = sum_q w_q rho_q phi_i(x_q) phi_j(x_q) / (sigma_i sigma_j),          moment0 = sum_q w_q rho_q,

is a finite sum over the composite Gauss-Legendre rule the library builds.  It is evaluated here in 80-bit np.longdouble
(eps = 2^-63), which pins every output of a device solve AT THE MULTIPLIERS THE DEVICE RETURNED without having to agree on the
iteration path.  Next to every value comes its first-order condition scale (the sum of the absolute values of the terms, each
weighted with c_q = 1 + sum_i |phi_i lambda_i| / sigma_i for the rounding of the exponent); an error is reported in UNITS of
u * scale, u = 2^-53.

Every routine takes the working dtype: np.longdouble gives the reference, np.float64 the *twin* -- the same sums in plain fp64
with NumPy's leggauss nodes.  The twin only calibrates tolerances (tests/test_maxent_exact_cpu.py); no device result is ever
compared with it.  Nothing here imports the package, the device, or the oracle.
"""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53

LEGENDRE, MONOMIAL, FOURIER, SPLINE = "legendre", "monomial", "fourier", "spline"
_DEFAULT_REF = {LEGENDRE: (-1.0, 1.0), MONOMIAL: (0.0, 1.0), FOURIER: (0.0, 2 * np.pi), SPLINE: (0.0, 1.0)}


class Desc:
    """Plain description of a moments object: kind, size of the underlying family, domain, ref_domain, log and the matrix of a
    TransformedMoments ([out_size, size] or None).  shift / scale are the fp64 values the package computes (moments.py)."""

    def __init__(self, kind, size, domain, ref_domain=None, log=False, matrix=None):
        self.kind = kind
        self.size = int(size)
        self.domain = (float(domain[0]), float(domain[1]))
        self.ref_domain = tuple(float(v) for v in (_DEFAULT_REF[kind] if ref_domain is None else ref_domain))
        self.log = bool(log)
        self.matrix = None if matrix is None else np.ascontiguousarray(matrix, dtype=np.float64)
        lo, hi = (np.log(self.domain[0]), np.log(self.domain[1])) if log else self.domain
        width = max(hi - lo, 1e-15)
        self.scale = float((self.ref_domain[1] - self.ref_domain[0]) / width)
        self.shift = float(lo)
        self.out_size = self.size if matrix is None else self.matrix.shape[0]


# ---------------------------------------------------------------------------------------------------------------------------
# quadrature
# ---------------------------------------------------------------------------------------------------------------------------
_GL_CACHE = {}


def _legendre_pn(n, z):
    """P_n(z), P_{n-1}(z) by the three-term recurrence, in the dtype of z"""
    p1, p2 = np.ones_like(z), np.zeros_like(z)
    for j in range(1, n + 1):
        p1, p2 = ((2 * j - 1) * z * p1 - (j - 1) * p2) / j, p1
    return p1, p2


def gauss_legendre_ld(n):
    """Nodes and weights of the n-point Gauss-Legendre rule on [-1, 1] in long double: Newton on P_n from NumPy's fp64 nodes,
    w = 2 / ((1 - z^2) P_n'(z)^2).  Nodes ascending and exactly antisymmetric."""
    if n not in _GL_CACHE:
        z = np.polynomial.legendre.leggauss(n)[0].astype(LD)
        for _ in range(4):                               # quadratic convergence from 1e-16: two steps suffice
            p1, p2 = _legendre_pn(n, z)
            pp = n * (z * p1 - p2) / (z * z - 1)
            z = z - p1 / pp
        z = (z - z[::-1]) / 2
        p1, p2 = _legendre_pn(n, z)
        pp = n * (z * p1 - p2) / (z * z - 1)
        w = 2 / ((1 - z * z) * pp * pp)
        _GL_CACHE[n] = (z, (w + w[::-1]) / 2)
    z, w = _GL_CACHE[n]
    return z.copy(), w.copy()


def _gauss(n, dtype):
    if dtype is LD:
        return gauss_legendre_ld(n)
    return np.polynomial.legendre.leggauss(n)


def composite_rule(a, b, n_intervals, degree, dtype=LD):
    """The library's rule: h = (b - a) / n, interval k = [a + k h, a + (k + 1) h] with the last one ending at b,
    x = (g + 1) / 2 (hi - lo) + lo, w = g_w (hi - lo) / 2 -- carried out in `dtype` from the fp64 a, b."""
    gx, gw = _gauss(degree, dtype)
    a, b = dtype(float(a)), dtype(float(b))
    h = (b - a) / n_intervals
    k = np.arange(n_intervals).astype(dtype)
    lo = a + k * h
    hi = a + (k + 1) * h
    hi[-1] = b
    x = (gx[None, :] + 1) / 2 * (hi - lo)[:, None] + lo[:, None]
    w = gw[None, :] * (hi - lo)[:, None] / 2
    return x.ravel(), w.ravel()


# ---------------------------------------------------------------------------------------------------------------------------
# basis
# ---------------------------------------------------------------------------------------------------------------------------
def _transform(desc, x, dtype):
    """t = (x - shift) * scale + ref0 (after log) in `dtype`; outside = the fp64 decision of the oracle's transform."""
    x = np.atleast_1d(np.asarray(x))
    x64 = x.astype(np.float64)
    with np.errstate(all="ignore"):
        v64 = np.log(x64) if desc.log else x64
        t64 = (v64 - desc.shift) * desc.scale + desc.ref_domain[0]
        outside = (t64 < desc.ref_domain[0]) | (t64 > desc.ref_domain[1]) | np.isnan(t64)
        xd = x.astype(dtype)
        v = np.log(xd) if desc.log else xd
        t = (v - dtype(desc.shift)) * dtype(desc.scale) + dtype(desc.ref_domain[0])
    return t, outside


def _family(desc, t, size, dtype):
    """rows [n, size] of the underlying family at transformed t (finite, inside the reference domain)"""
    n = t.shape[0]
    v = np.empty((size, n), dtype=dtype)
    v[0] = 1
    if desc.kind == LEGENDRE:
        if size > 1:
            v[1] = t
        for i in range(2, size):
            v[i] = (v[i - 1] * t * (2 * i - 1) - v[i - 2] * (i - 1)) / i
    elif desc.kind == MONOMIAL:
        for i in range(1, size):
            v[i] = v[i - 1] * t
    elif desc.kind == FOURIER:
        for i in range(1, size):
            k = (i + 1) // 2
            v[i] = np.cos(k * t) if i % 2 else np.sin(k * t)
    elif desc.kind == SPLINE:
        ns = desc.size - 3
        knots = np.clip(np.arange(-3, ns + 4), 0, ns).astype(dtype) / dtype(ns)
        u = (t - dtype(desc.ref_domain[0])) / (dtype(desc.ref_domain[1]) - dtype(desc.ref_domain[0]))
        nk = len(knots)
        span = np.clip(np.floor(u * ns).astype(np.int64), 0, ns - 1) + 3           # knots[span] <= u <= knots[span + 1]
        N = np.zeros((nk - 1, n), dtype=dtype)
        N[span, np.arange(n)] = 1
        for p in range(1, 4):                                                      # Cox-de Boor, 0 / 0 = 0
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
    return v.T


def basis(desc, x, size, dtype=LD):
    """phi [n, size] and |phi| [n, size] (for a transformed basis |L| . |phi_underlying|) at the points x; rows of masked
    points (the oracle's fp64 decision) are NaN."""
    t, outside = _transform(desc, x, dtype)
    ok = ~outside
    und_size = desc.size if desc.matrix is not None else size
    und = np.full((t.shape[0], und_size), np.nan, dtype=dtype)
    if ok.any():
        und[ok] = _family(desc, t[ok], und_size, dtype)
    if desc.matrix is None:
        return und, np.abs(und)
    L = desc.matrix[:size].astype(dtype)
    return und @ L.T, np.abs(und) @ np.abs(L).T


def basis_ld(desc, x, size):
    return basis(desc, x, size, LD)


# ---------------------------------------------------------------------------------------------------------------------------
# functional
# ---------------------------------------------------------------------------------------------------------------------------
def _rho(phi, aphi, ls, dtype):
    with np.errstate(all="ignore"):
        e = -(phi @ ls)
        rho = np.exp(np.minimum(np.maximum(e, dtype(-200)), dtype(200)))
        c = 1 + aphi @ np.abs(ls)
    return e, rho, c


def _sym(upper):
    """mirror the upper triangle: exactly symmetric"""
    return np.triu(upper) + np.triu(upper, 1).T


def functional(desc, mu, sigma, lam, a, b, n_intervals, degree, dtype=LD, hess=True):
    """dict with F, g, H, moment0 and the condition scales F_scale, g_scale, H_scale, m_scale, plus the exponents e at the
    quadrature points and c_max = max_q c_q (the scales are first-order: they mean something while u c_max << 1).
    R1 = len(lam)."""
    n_intervals = n_intervals if n_intervals > 0 else 64
    degree = degree if degree > 0 else 21
    lam = np.asarray(lam, dtype=np.float64).astype(dtype)
    R1 = len(lam)
    mu = np.asarray(mu, dtype=np.float64)[:R1].astype(dtype)
    sigma = np.asarray(sigma, dtype=np.float64)[:R1].astype(dtype)
    x, w = composite_rule(a, b, n_intervals, degree, dtype)
    phi, aphi = basis(desc, x, R1, dtype)
    ls = lam / sigma
    e, rho, c = _rho(phi, aphi, ls, dtype)
    wr = w * rho
    wrc = wr * c
    m0 = np.sum(wr)
    lin = mu * ls
    out = dict(e=e, c_max=np.max(c), moment0=m0, m_scale=np.sum(wrc), F=np.sum(lin) + m0, F_scale=np.sum(np.abs(lin)) + np.sum(wrc),
               g=mu / sigma - (wr @ phi) / sigma, g_scale=np.abs(mu / sigma) + (wrc @ aphi) / sigma, n_quad=len(x))
    if hess:
        ps, aps = phi / sigma[None, :], aphi / sigma[None, :]
        out["H"] = _sym((ps * wr[:, None]).T @ ps)
        out["H_scale"] = _sym((aps * wrc[:, None]).T @ aps)
    return out


def functional_ld(desc, mu, sigma, lam, a, b, n_intervals, degree, hess=True):
    return functional(desc, mu, sigma, lam, a, b, n_intervals, degree, LD, hess)


def functional_f64(desc, mu, sigma, lam, a, b, n_intervals, degree, hess=True):
    """the twin: the same sums in plain fp64 with np.polynomial.legendre.leggauss nodes (calibration only)"""
    return functional(desc, mu, sigma, lam, a, b, n_intervals, degree, np.float64, hess)


def density(desc, lam, sigma, x, dtype=LD):
    """rho(x) = exp(clip(-phi(x) . lambda / sigma, +-200)), its pointwise scale rho(x) c(x) and the unclipped exponent;
    NaN at masked points"""
    lam = np.asarray(lam, dtype=np.float64).astype(dtype)
    sigma = np.asarray(sigma, dtype=np.float64)[:len(lam)].astype(dtype)
    phi, aphi = basis(desc, x, len(lam), dtype)
    e, rho, c = _rho(phi, aphi, lam / sigma, dtype)
    return rho, rho * c, e


def density_ld(desc, lam, sigma, x):
    return density(desc, lam, sigma, x, LD)


def integrate(desc, lam, sigma, lo, hi, degree, dtype=LD):
    """integral of the density over [lo_i, hi_i] by one `degree`-point Gauss-Legendre rule per interval, and its scale
    sum |w| rho c"""
    gx, gw = _gauss(degree, dtype)
    lo = np.atleast_1d(np.asarray(lo, dtype=np.float64)).astype(dtype)
    hi = np.atleast_1d(np.asarray(hi, dtype=np.float64)).astype(dtype)
    x = (gx[None, :] + 1) / 2 * (hi - lo)[:, None] + lo[:, None]
    w = gw[None, :] * (hi - lo)[:, None] / 2
    rho, scale, _ = density(desc, lam, sigma, x.ravel(), dtype)
    with np.errstate(all="ignore"):
        val = np.sum(w * rho.reshape(x.shape), axis=1)
        sc = np.sum(np.abs(w) * scale.reshape(x.shape), axis=1)
    return val, sc


def integrate_ld(desc, lam, sigma, lo, hi, degree):
    return integrate(desc, lam, sigma, lo, hi, degree, LD)


# ---------------------------------------------------------------------------------------------------------------------------
# errors in units of u * scale
# ---------------------------------------------------------------------------------------------------------------------------
def units(got, ref, scale):
    """max over the entries of |got - ref| / (u scale), in long double.  Entries where the reference is not finite must
    match exactly (same NaN positions, same infinities): a mismatch gives inf."""
    got = np.atleast_1d(np.asarray(got)).astype(LD)
    ref = np.atleast_1d(np.asarray(ref)).astype(LD)
    scale = np.broadcast_to(np.atleast_1d(np.asarray(scale)).astype(LD), ref.shape)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    fin = np.isfinite(ref)
    worst = LD(0)
    if not np.array_equal(got[~fin], ref[~fin], equal_nan=True) or not np.all(np.isfinite(got[fin])):
        return float("inf")
    if fin.any():
        err = np.abs(got[fin] - ref[fin])
        s = U * scale[fin]
        with np.errstate(all="ignore"):
            q = np.where(err == 0, LD(0), err / s)
        worst = np.max(q)
    return float(worst)
