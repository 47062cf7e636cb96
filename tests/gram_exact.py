"""Extended-precision reference of the two fp64 matrix-core contractions -- TEST INFRASTRUCTURE, plain NumPy, a sibling of
tests/accum_exact.py (whose rows, transform and unit_errors it uses).  Nothing here imports the package, the device or the oracle.

Component covariance (mlmc_xcov_create).  The fp64 values f~ = fl(f - a), c~ = fl(c - a) are part of the contract (the kernel
subtracts the shift in fp64 on the way into LDS); everything after them is long double.  A NaN in any of the 2 M values of a
sample drops it from the whole matrix.  Per kept sample, by the DEFINITION and not by the kernel's identities,

    Y = f~ f~^T - c~ c~^T   (level 0: f~ f~^T),      s = sum Y,      sp = sum Y o Y,

formed per sample in chunks of samples (expanding Y o Y into three Grams would cancel in long double when f ~ c).  Scales:

    A = (|f~_i| + |c~_i|) (|f~_j| + |c~_j|),         S = sum A,      SP = sum A^2,

the scale tests/accum_exact.cov_sums uses: it bounds the terms of the definition and of (d_i s_j + s_i d_j) / 2 alike
(Y^2 + 2 |Y| A would be too tight: with f_i = 1, c_i = 0, f_j = 0, c_j = 1, Y is exactly 0 while the kernel's terms are +-1).
Where a scale is exactly zero the value must be exactly zero (accum_exact.unit_errors).

Bootstrap (mlmc_bootstrap_accum).  For one chunk and integer weights w [n] of one replicate

    n = sum w keep,   s = sum w d,   sp = sum w d^2,   S = sum w (a + E),   SP = sum w (d^2 + 2 |d| (a + E))

with the rows d = phi(f) - phi(c), a = |phi(f)| + |phi(c)| and the log budget E of accum_exact (level_sums / _side).  The
weights are integers and enter exactly.  The shared-basis layout ANDs the keep over the components; the per-component layout is
this function on the one-component chunk of every row with that component's own Desc.

Twins (np.float64, calibration only -- no device result is ever compared with a twin):
    covariance   A  the definition in fp64;   B  the identities 1/2 (D^T S + S^T D), 1/4 (G1 + G1^T + 2 G2) in fp64
    bootstrap    A / B  the row variants of accum_exact, weighted in fp64
"""
import numpy as np

from tests import accum_exact as ax

LD = ax.LD
_CHUNK = 1 << 21                          # elements of one [samples, M, M] block


class Sums:
    """n, n_rm [L]; s, sp, S, SP [L, M * M] (row i * M + j) in the working dtype"""


# ---------------------------------------------------------------------------------------------------------------------------
# component covariance
# ---------------------------------------------------------------------------------------------------------------------------
def xcov_kept(fine, coarse, shift):
    """keep [n] and the fp64 shifted values f~ [M, n_keep], c~ [M, n_keep] | None of one level"""
    f = np.asarray(fine, dtype=np.float64)
    c = None if coarse is None else np.asarray(coarse, dtype=np.float64)
    a = np.zeros(f.shape[0]) if shift is None else np.asarray(shift, dtype=np.float64)
    bad = np.isnan(f).any(axis=0)
    if c is not None:
        bad |= np.isnan(c).any(axis=0)
    keep = ~bad
    return keep, f[:, keep] - a[:, None], None if c is None else c[:, keep] - a[:, None]


def xcov_definition(F, C, dtype=LD):
    """s, sp, S, SP [M, M] of the kept shifted values by the definition, per sample, in `dtype`"""
    M, n = F.shape
    s, sp, S, SP = (np.zeros((M, M), dtype=dtype) for _ in range(4))
    b = max(1, _CHUNK // (M * M))
    for k0 in range(0, n, b):
        Fb = F[:, k0:k0 + b].T.astype(dtype)
        Y = Fb[:, :, None] * Fb[:, None, :]
        A = np.abs(Fb)
        if C is not None:
            Cb = C[:, k0:k0 + b].T.astype(dtype)
            Y -= Cb[:, :, None] * Cb[:, None, :]
            A = A + np.abs(Cb)
        AA = A[:, :, None] * A[:, None, :]
        s += Y.sum(axis=0)
        sp += (Y * Y).sum(axis=0)
        S += AA.sum(axis=0)
        SP += (AA * AA).sum(axis=0)
    return s, sp, S, SP


def _gram(X, Y):
    """sum_k X[i, k] Y[j, k] in fp64 without BLAS: NumPy's pairwise sum inside a chunk of samples, the chunks in order"""
    M, n = X.shape
    out = np.zeros((M, M))
    b = max(1, _CHUNK // (M * M))
    for k0 in range(0, n, b):
        out += (X[:, None, k0:k0 + b] * Y[None, :, k0:k0 + b]).sum(axis=-1)
    return out


def xcov_identities(F, C, g2_weight=2.0):
    """s, sp [M, M] in fp64 from d = f~ - c~, s = f~ + c~: the identities the kernel is built on (twin B).  g2_weight: 2, except
    in the deliberately flawed twin of tests/test_gram_exact_cpu.py."""
    if C is None:
        return _gram(F, F), _gram(F * F, F * F)
    D, Sm = F - C, F + C
    v0 = _gram(D, Sm)
    g1, g2 = _gram(D * D, Sm * Sm), _gram(D * Sm, D * Sm)
    return 0.5 * (v0 + v0.T), 0.25 * (g1 + g1.T + g2_weight * g2)


def xcov_sums(levels, shift, dtype=LD, variant="A"):
    """levels: [(fine [M, n], coarse [M, n] | None)] raw values, shift [M] | None -> Sums.  dtype=LD: the reference (variant
    "A", the definition); np.float64: twin "A" (the definition) or "B" (the identities; its S, SP are zero -- take the
    reference's)."""
    L, M = len(levels), np.asarray(levels[0][0]).shape[0]
    out = Sums()
    out.n, out.n_rm = np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64)
    out.s, out.sp, out.S, out.SP = (np.zeros((L, M * M), dtype=dtype) for _ in range(4))
    for l, (f, c) in enumerate(levels):
        keep, F, C = xcov_kept(f, c, shift)
        out.n[l], out.n_rm[l] = keep.sum(), (~keep).sum()
        if variant == "A":
            s, sp, S, SP = xcov_definition(F, C, dtype)
            out.S[l], out.SP[l] = S.reshape(-1), SP.reshape(-1)
        else:
            assert dtype is np.float64
            s, sp = xcov_identities(F, C)
        out.s[l], out.sp[l] = s.reshape(-1), sp.reshape(-1)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# bootstrap
# ---------------------------------------------------------------------------------------------------------------------------
def kept_rows(desc, fine, coarse, dtype=LD, variant="A"):
    """keep [n] (the AND over the M components of fine and coarse) and, over the kept samples, d [M * R, n_keep] and the scale
    rows a + E [M * R, n_keep] (row m * R + r) of one chunk"""
    f = np.atleast_2d(np.asarray(fine, dtype=np.float64))
    c = None if coarse is None else np.atleast_2d(np.asarray(coarse, dtype=np.float64))
    keep = np.ones(f.shape[1], dtype=bool)
    for side in (f,) if c is None else (f, c):
        for m in range(side.shape[0]):
            keep &= ax.transform(desc, side[m], np.float64)[1]
    pf, Ef = ax._side(desc, f, keep, dtype, variant)
    if c is None:
        d, aE = pf, np.abs(pf) + Ef
    else:
        pc, Ec = ax._side(desc, c, keep, dtype, variant)
        d, aE = pf - pc, np.abs(pf) + np.abs(pc) + Ef + Ec
    K = f.shape[0] * desc.size
    return keep, d.reshape(K, -1), aE.reshape(K, -1)


def weighted_sums(desc, fine, coarse, w, dtype=LD, variant="A", rows=None):
    """w: integer weights [n] of one replicate or [nb, n] of several -> n [nb] (int64), s, sp, S, SP [nb, M * R] in `dtype`.
    rows: kept_rows(desc, fine, coarse, dtype, variant) when the caller has them already."""
    w = np.atleast_2d(np.asarray(w))
    assert w.dtype.kind in "iu" and np.all(w >= 0)
    keep, d, aE = kept_rows(desc, fine, coarse, dtype, variant) if rows is None else rows
    assert w.shape[1] == keep.shape[0]
    wk = w[:, keep].astype(np.int64)
    n = wk.sum(axis=1)
    dd = d * d
    cond = dd + 2 * np.abs(d) * aE
    out = [np.zeros((w.shape[0], d.shape[0]), dtype=dtype) for _ in range(4)]
    for b in range(w.shape[0]):
        wb = wk[b].astype(dtype)[None, :]                # integers below 2^31: exact in either dtype
        for dst, src in zip(out, (d, dd, aE, cond)):
            dst[b] = (wb * src).sum(axis=-1)
    return (n, *out)
