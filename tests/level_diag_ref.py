"""Reference of the level diagnostics (mlmc_level_diagnostics): the nine statistics in 80-bit long double, and the scales of
the accuracy gate.

Every sum is taken of values shifted by one SAMPLE first (d0 = x - x[n // 2], then d = d0 - mean(d0)): a plain long-double mean of
values near 1e6 is itself wrong by 1e4 units of the third central sum; the shifted form agrees with exact rational arithmetic
to 0.0004 units on 4001 such samples (test_level_diagnostics_cpu.py gates it at 0.1)."""
import numpy as np

LD = np.longdouble
N_STAT = 9
GATE_SUM = 32.0          # units of 2^-53 sum |x - mean|^k (co-moment: sum |f - mean f| |c - mean c|)
GATE_MEAN = 4.0          # units of 2^-53 (|mean| + sd)
U = 2.0 ** -53


def _centred(x):
    """x [n] float64 -> (mean, d = x - mean) in long double"""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    pivot = x[x.size // 2]
    d0 = x - pivot
    shift = np.sum(d0) / LD(x.size)
    return pivot + shift, d0 - shift


def stats(f, c=None):
    """One (level, component): fine [n], coarse [n] | None -> (n, n_rm, stats [9] long double, scale [9] long double).
    scale[s] is what the error of stats[s] is measured in: |mean| + sd for the means, sum |d|^k for the central sums."""
    f = np.asarray(f, dtype=np.float64)
    keep = ~np.isnan(f)
    if c is not None:
        c = np.asarray(c, dtype=np.float64)
        keep &= ~np.isnan(c)
    n = int(np.count_nonzero(keep))
    out = np.full(N_STAT, np.nan, dtype=LD)
    scale = np.full(N_STAT, np.nan, dtype=LD)
    if n == 0:
        return n, f.size - n, out, scale
    fk = f[keep]
    y = fk if c is None else fk - c[keep]                  # the fp64 difference, as estimate_mean forms it
    mean_y, dy = _centred(y)
    ay = np.abs(dy)
    out[0:4] = mean_y, np.sum(dy ** 2), np.sum(dy ** 3), np.sum(dy ** 4)
    scale[0:4] = np.abs(mean_y) + np.sqrt(out[1] / n), np.sum(ay ** 2), np.sum(ay ** 3), np.sum(ay ** 4)
    mean_f, df = _centred(fk)
    out[4:6] = mean_f, np.sum(df ** 2)
    scale[4:6] = np.abs(mean_f) + np.sqrt(out[5] / n), out[5]
    if c is not None:
        mean_c, dc = _centred(c[keep])
        out[6:9] = mean_c, np.sum(dc ** 2), np.sum(df * dc)
        scale[6:9] = np.abs(mean_c) + np.sqrt(out[7] / n), out[7], np.sum(np.abs(df) * np.abs(dc))
    return n, f.size - n, out, scale


def levels_stats(levels):
    """levels: [(fine [M, n], coarse [M, n] | None)] -> n, n_rm [L, M] int64, stats, scale [L, M, 9] long double"""
    L, M = len(levels), levels[0][0].shape[0]
    n = np.zeros((L, M), dtype=np.int64)
    n_rm = np.zeros((L, M), dtype=np.int64)
    out = np.zeros((L, M, N_STAT), dtype=LD)
    scale = np.zeros((L, M, N_STAT), dtype=LD)
    for l, (f, c) in enumerate(levels):
        for m in range(M):
            n[l, m], n_rm[l, m], out[l, m], scale[l, m] = stats(f[m], None if c is None else c[m])
    return n, n_rm, out, scale


def units(got, want, scale):
    """Error of got [..., 9] (float64) against want in the units of the gate: 2^-53 scale.  An entry whose reference is NaN
    must be NaN (-> 0 units, else inf); a zero scale demands the exact value."""
    got = np.asarray(got, dtype=np.float64).astype(LD)
    err = np.abs(got - want)
    with np.errstate(all="ignore"):
        u = np.where(err == 0, LD(0), err / (LD(U) * scale))
    nan_ref = np.isnan(want)
    u = np.where(nan_ref, np.where(np.isnan(got), LD(0), LD(np.inf)), u)
    u = np.where(~nan_ref & np.isnan(got), LD(np.inf), u)
    return u.astype(np.float64)


MEAN_IDX = (0, 4, 6)
SUM_IDX = (1, 2, 3, 5, 7, 8)


def worst_units(got, want, scale):
    """-> (worst error of a mean, worst error of a central sum), in units of the gate"""
    u = units(got, want, scale)
    return float(np.max(u[..., MEAN_IDX])), float(np.max(u[..., SUM_IDX]))
