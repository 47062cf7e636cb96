"""Long-double reference, fp64 twins, cases and tolerances of the component-covariance bootstrap (mlmc_bootstrap_create_xcov) --
TEST INFRASTRUCTURE, plain NumPy, a sibling of tests/gram_exact.py (whose xcov_kept and LD it uses).  Nothing here imports the
package or the device.

Definition (include/mlmc_hip.h).  For one chunk [M, n], a shift a and integer weights w [n] of one replicate, with the fp64 values
f~ = fl(f - a), c~ = fl(c - a) (part of the contract, as for mlmc_xcov_create) and keep_i = 0 when any of the 2 M values of sample
i is NaN:

    n = sum w keep,    s1[m] = sum w keep (f~_m - c~_m),    s2[i, j] = sum w keep (f~_i f~_j - c~_i c~_j)
    U1[m] = sum w keep (|f~_m| + |c~_m|),                   U2[i, j] = sum w keep (|f~_i f~_j| + |c~_i c~_j|)

(level 0: no coarse terms).  Everything after f~, c~ is long double in the reference; the weights are integers and enter exactly.
An error is measured in units of 2^-53 U1 / 2^-53 U2; where a scale is exactly zero the value must be exactly zero
(accum_exact.unit_errors).

Twins (np.float64, calibration only -- no device result is ever compared with a twin):
    A  every term in fp64, the samples added one after the other
    B  every term in fp64, slices of 512 samples added one after the other, then the slices in order
flaw=... gives the deliberately broken variants of tests/test_xcov_boot_cpu.py.
"""
import numpy as np

from tests import accum_exact as ax
from tests import gram_exact as gx

LD = gx.LD
SLICE = 512


def _sum(x, variant):
    """sum over the last axis: 'ref' NumPy's sum in the array's dtype, 'A' sequential, 'B' sequential in slices of SLICE, then
    the slices in order"""
    if x.shape[-1] == 0:
        return np.zeros(x.shape[:-1], dtype=x.dtype)
    if variant == "ref":
        return x.sum(axis=-1)
    if variant == "A":
        return np.cumsum(x, axis=-1)[..., -1]
    parts = [np.cumsum(x[..., k:k + SLICE], axis=-1)[..., -1] for k in range(0, x.shape[-1], SLICE)]
    return np.cumsum(np.stack(parts, axis=-1), axis=-1)[..., -1]


def weighted_sums(fine, coarse, shift, w, dtype=LD, variant="ref", flaw=None):
    """w: integer weights [nb, n] (or [n]) -> n [nb] int64, s1, U1 [nb, M], s2, U2 [nb, M, M] in `dtype`.
    flaw: None | 'no_coarse' (the coarse term is dropped) | 'keep_nan' (a sample with a NaN is kept, the NaN counted as 0) |
    'coarse_unshifted' (the shift is forgotten on the coarse side)"""
    w = np.atleast_2d(np.asarray(w))
    assert w.dtype.kind in "iu" and np.all(w >= 0)
    f = np.asarray(fine, dtype=np.float64)
    c = None if coarse is None else np.asarray(coarse, dtype=np.float64)
    M, n = f.shape
    assert w.shape[1] == n
    a = np.zeros(M) if shift is None else np.asarray(shift, dtype=np.float64)
    keep = ~np.isnan(f).any(axis=0)
    if c is not None:
        keep &= ~np.isnan(c).any(axis=0)
    if flaw == "keep_nan":
        f = np.nan_to_num(f, nan=0.0)
        c = None if c is None else np.nan_to_num(c, nan=0.0)
        keep = np.ones(n, dtype=bool)
    with np.errstate(invalid="ignore"):
        F = np.where(keep, f - a[:, None], 0.0).astype(dtype)             # a dropped sample contributes exact zeros
        C = None
        if c is not None and flaw != "no_coarse":
            C = np.where(keep, c - (0.0 if flaw == "coarse_unshifted" else a[:, None]), 0.0).astype(dtype)
    wk = (w * keep[None, :]).astype(np.int64)
    nb = w.shape[0]
    cnt = wk.sum(axis=1)
    s1, U1 = (np.zeros((nb, M), dtype=dtype) for _ in range(2))
    s2, U2 = (np.zeros((nb, M, M), dtype=dtype) for _ in range(2))
    D = F if C is None else F - C
    A1 = np.abs(F) if C is None else np.abs(F) + np.abs(C)
    for b in range(nb):
        wb = wk[b].astype(dtype)[None, :]                                  # integers below 2^31: exact in either dtype
        s1[b] = _sum(wb * D, variant)
        U1[b] = _sum(wb * A1, "ref")
        for i in range(M):
            Y = F[i][None, :] * F[i:]
            A2 = np.abs(Y)
            if C is not None:
                Z = C[i][None, :] * C[i:]
                Y = Y - Z
                A2 = A2 + np.abs(Z)
            s2[b, i, i:] = _sum(wb * Y, variant)
            U2[b, i, i:] = _sum(wb * A2, "ref")
            s2[b, i:, i] = s2[b, i, i:]
            U2[b, i:, i] = U2[b, i, i:]
    return cnt, s1, s2, U1, U2


def units(got, ref, scale):
    """worst error of `got` against `ref` in units of 2^-53 scale"""
    return float(np.max(ax.unit_errors(got, ref, scale))) if np.size(ref) else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------
def make_chunk(M, n, seed, pair, offset=0.0, nan=True):
    """fine [M, n], coarse [M, n] | None: correlated normals around offset + 0.1 m, the coarse values close to the fine ones;
    nan: one NaN in a fine and (pair) one in a coarse component, at different samples"""
    rng = np.random.default_rng([seed, M, n, int(pair)])
    z = rng.normal(size=(M, n))
    f = offset + 0.1 * np.arange(M)[:, None] + z + 0.5 * z[::-1]
    c = f + 0.3 * rng.normal(size=(M, n)) if pair else None
    if nan and n >= 8:
        f[M // 2, 5::97] = np.nan
        if pair:
            c[M - 1, 3::61] = np.nan
    return f, c


def make_shift(M, kind, offset=0.0):
    """None ('zero') or M finite values near the mean of make_chunk's data ('mean')"""
    if kind == "zero":
        return None
    return offset + 0.1 * np.arange(M) + 0.0123


def multinomial_weights(n, sizes, seed):
    """[len(sizes), n] weights under NumPy's own multinomial: the law of the device's weights, not its draws"""
    rng = np.random.default_rng([77, seed, n])
    return np.stack([rng.multinomial(int(s), np.full(n, 1.0 / n)) for s in sizes]).astype(np.int64)


# calibration cases: (name, M, n, offset).  The shapes cover one and several 512-sample slices and tiles; offset = 100 with the
# 'mean' shift is the regime the shift exists for (|mean| >> std), with the 'zero' shift the one it spares the sums.
CALIBRATION = [("M3_n513", 3, 513, 0.0), ("M5_n4097", 5, 4097, 0.0), ("M12_n8197", 12, 2 * 4096 + 5, 0.0),
               ("M4_n4097_offset", 4, 4097, 100.0)]
CLASSES = ("level0", "pair")
QUANTITIES = ("s1", "s2")


def calibration_sizes(n):
    return [n, n // 2, max(1, n // 7)]


# Worst error of twins A and B against the long-double reference in units of 2^-53 * scale over CALIBRATION x both shifts x the
# three replicates of calibration_sizes; measured and asserted by tests/test_xcov_boot_cpu.py::test_twin_calibration_table.
XCOV_BOOT_TWIN_UNITS = {
    # level 0: M12_n8197 (A: 8197 terms of one sign on the diagonal, added one after the other), M4_n4097_offset / M3_n513 (B)
    "level0": dict(s1=(29.9, 4.62), s2=(47.0, 15.4)),
    # pair: M12_n8197 (A), M3_n513 (B): the differences change sign, the partial sums stay far below the scale
    "pair": dict(s1=(0.139, 0.076), s2=(1.90, 0.537)),
}


def tolerance(cls, quantity):
    """max(16, 4 x the worse twin) units: the project's rule (tests/accum_cases.tolerance)"""
    a, b = XCOV_BOOT_TWIN_UNITS[cls][quantity]
    return max(16.0, 4.0 * max(a, b))


# ---------------------------------------------------------------------------------------------------------------------------
# device shapes (tests/test_gpu_xcov_boot.py): each axis swept with the others small, plus two mixed cases.
# 62 is the largest M whose 1 + M + M (M + 1) / 2 columns fit one group of 2048, 63 the first that needs two.
# ---------------------------------------------------------------------------------------------------------------------------
M_SWEEP = [1, 2, 5, 12, 16, 17, 33, 62, 63]
N_SWEEP = [1, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 2 * 4096 + 5]
B_SWEEP = [1, 63, 64, 65, 257]


def device_shapes():
    """[(M, n, B)]"""
    out = [(M, 130, 3) for M in M_SWEEP]
    out += [(3, n, 3) for n in N_SWEEP]
    out += [(2, 70, B) for B in B_SWEEP]
    out += [(17, 4097, 65), (63, 513, 5)]
    return out
