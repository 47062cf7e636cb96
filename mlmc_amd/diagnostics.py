"""Per-level MLMC convergence diagnostics of every component (host side; pure NumPy, needs no device).

The standard convergence tests of an MLMC level hierarchy (Giles' `mlmc_test`): kurtosis of the level differences, the fine
and coarse statistics of a level side by side, their correlation, the telescoping-consistency check between neighbouring
levels and the decay rates alpha, beta, gamma.  The central sums come from one call of the device
(`quantity_estimate.level_diagnostics`, mlmc_amd/csrc/level_diag.hip); everything here is O(L M) arithmetic on them.
"""
import collections

import numpy as np

# order of the statistics per (level, component): MLMC_DIAG_NSTAT of include/mlmc_hip.h
STAT_NAMES = ("mean_y", "M2_y", "M3_y", "M4_y", "mean_f", "M2_f", "mean_c", "M2_c", "C_fc")
N_STAT = len(STAT_NAMES)

Rates = collections.namedtuple("Rates", "alpha beta gamma bias")


def _slope(x, y):
    """Unweighted least-squares slope of y against x over the finite pairs; NaN with fewer than two of them."""
    ok = np.isfinite(x) & np.isfinite(y)
    if np.count_nonzero(ok) < 2:
        return np.nan
    x, y = x[ok], y[ok]
    dx = x - np.mean(x)
    den = np.sum(dx * dx)
    if den == 0.0:
        return np.nan
    return float(np.sum(dx * (y - np.mean(y))) / den)


class LevelDiagnostics:
    """[L, M] arrays of the per-level statistics of M components (from_central_sums documents the fields), the level steps
    h_l [L] and the costs per sample n_ops [L] (None when not given)."""

    FIELDS = ("n_samples", "mean_diff", "var_diff", "skew_diff", "kurtosis_diff", "mean_fine", "var_fine", "mean_coarse",
              "var_coarse", "corr_fine_coarse", "consistency")

    def __init__(self, level_steps=None, n_ops=None, **fields):
        for name in self.FIELDS:
            setattr(self, name, fields[name])
        self.level_steps = level_steps
        self.n_ops = n_ops

    @property
    def mlmc_mean(self):
        """[M]: sum over the levels of mean_diff, the MLMC estimate of the mean."""
        return np.sum(self.mean_diff, axis=0)

    @property
    def mlmc_var(self):
        """[M]: sum over the levels of var_diff / n, the variance of that estimate."""
        with np.errstate(all="ignore"):
            return np.sum(self.var_diff / self.n_samples, axis=0)

    def rates(self):
        """Rates(alpha [M], beta [M], gamma, bias [M]): |mean_diff| ~ h^alpha and var_diff ~ h^beta fitted over the levels
        1 .. L - 1 (a level with a zero or non-finite entry is left out of that component's fit; fewer than two levels
        left: NaN), cost per sample n_ops ~ h^-gamma over all levels (NaN without n_ops), and the remaining bias
        |mean_diff[L - 1]| / ((h_{L-2} / h_{L-1})^alpha - 1) (NaN for alpha <= 0).  NaN without level steps."""
        L, M = self.mean_diff.shape
        alpha, beta, bias = np.full(M, np.nan), np.full(M, np.nan), np.full(M, np.nan)
        gamma = np.nan
        if self.level_steps is None:
            return Rates(alpha, beta, gamma, bias)
        with np.errstate(all="ignore"):
            log_h = np.log(self.level_steps)
            log_mean = np.log(np.abs(self.mean_diff))              # log 0 = -inf: not finite, left out by _slope
            log_var = np.log(self.var_diff)
            for m in range(M):
                alpha[m] = _slope(log_h[1:], log_mean[1:, m])
                beta[m] = _slope(log_h[1:], log_var[1:, m])
            if self.n_ops is not None:
                gamma = -_slope(log_h, np.log(self.n_ops))
            if L >= 2:
                ratio = self.level_steps[L - 2] / self.level_steps[L - 1]
                bias = np.where(alpha > 0.0, np.abs(self.mean_diff[L - 1]) / (ratio ** alpha - 1.0), np.nan)
        return Rates(alpha, beta, gamma, bias)

    def flags(self, kurtosis_max=100.0, consistency_max=1.0):
        """bool [L, M]: the kurtosis of the level differences or the consistency check exceeds its limit (NaN compares
        false).  A kurtosis far above the Gaussian 3 says that the level variance rests on a few samples; a consistency
        check above 1 says that the coarse values of level l and the fine values of level l - 1 do not estimate the same
        mean (more than 3 standard errors apart): the telescoping sum is broken."""
        with np.errstate(invalid="ignore"):
            return (self.kurtosis_diff > kurtosis_max) | (self.consistency > consistency_max)


def from_central_sums(n, stats, level_steps=None, n_ops=None):
    """LevelDiagnostics from the kept-sample counts n [L, M] and the central sums stats [L, M, 9] (STAT_NAMES: means and
    central sums M_k = sum (x - mean)^k of the level differences y, of the fine and of the coarse values, and the co-moment
    C_fc; NaN where a level has none).  Fields, all [L, M]:

        n_samples                 int64 count of kept samples
        mean_diff, var_diff       mean of y, M2_y / (n - 1) (the convention of engine.level_stats)
        skew_diff, kurtosis_diff  m3 / m2^1.5, m4 / m2^2 with m_k = M_k / n (the biased forms of Giles' mlmc_test)
        mean_fine, var_fine       of the fine values;  mean_coarse, var_coarse: of the coarse values (NaN at level 0)
        corr_fine_coarse          C_fc / sqrt(M2_f M2_c)
        consistency               |mean_coarse[l] - mean_fine[l-1]| / (3 (sqrt(var_coarse[l] / n[l]) + sqrt(var_fine[l-1] / n[l-1])));
                                  NaN at level 0
    Any 0 / 0 (no or one kept sample, constant data) gives NaN, never an exception."""
    n = np.array(n, dtype=np.int64)
    stats = np.asarray(stats, dtype=np.float64)
    if n.ndim != 2 or stats.shape != n.shape + (N_STAT,):
        raise ValueError("from_central_sums: n must be [L, M] and stats [L, M, {}], got {} and {}".format(
            N_STAT, n.shape, stats.shape))
    L = n.shape[0]
    if level_steps is not None:
        level_steps = np.asarray(level_steps, dtype=np.float64).reshape(-1)
        if level_steps.shape != (L,):
            raise ValueError("from_central_sums: {} level steps for {} levels".format(level_steps.size, L))
    if n_ops is not None:
        n_ops = np.asarray(n_ops, dtype=np.float64).reshape(-1)
        if n_ops.shape != (L,):
            raise ValueError("from_central_sums: {} n_ops for {} levels".format(n_ops.size, L))
    mean_y, M2y, M3y, M4y, mean_f, M2f, mean_c, M2c, Cfc = (stats[..., s] for s in range(N_STAT))
    nf = n.astype(np.float64)
    with np.errstate(all="ignore"):
        m2 = M2y / nf
        var_fine, var_coarse = M2f / (nf - 1.0), M2c / (nf - 1.0)
        consistency = np.full(n.shape, np.nan)
        if L > 1:
            consistency[1:] = np.abs(mean_c[1:] - mean_f[:-1]) / (
                3.0 * (np.sqrt(var_coarse[1:] / nf[1:]) + np.sqrt(var_fine[:-1] / nf[:-1])))
        return LevelDiagnostics(
            level_steps=level_steps, n_ops=n_ops, n_samples=n, mean_diff=mean_y.copy(), var_diff=M2y / (nf - 1.0),
            skew_diff=(M3y / nf) / m2 ** 1.5, kurtosis_diff=(M4y / nf) / (m2 * m2), mean_fine=mean_f.copy(), var_fine=var_fine,
            mean_coarse=mean_c.copy(), var_coarse=var_coarse, corr_fine_coarse=Cfc / np.sqrt(M2f * M2c), consistency=consistency)
