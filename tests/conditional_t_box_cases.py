"""What the tests of the conditional box entries of the Student-t copula share (mlmc_copula_box_prob_tc_batch / _draws_tc_batch,
include/mlmc_hip.h): tests/test_conditional_t_box_cpu.py, tests/test_gpu_conditional_t_box.py,
tests/test_gpu_conditional_t_box_api.py.  Nothing here touches the device.

  ct_twin        the chain of the header in NumPy: tests/t_box_cases.t_twin on the limits (lo - shift) / (scale s), with the
                 operations of the header: one rounded subtraction, c = scale * s one rounded product, one IEEE division;
  scaled_limits  those limits of every point, [n, M], as the GPU tests hand them to the Gaussian entry;
  problem, CASES the small problems of the GPU tests: the shapes of tests/t_box_cases.SHAPES with nu, nu_c, R, B spread over them;
  block_law      mu, r and the Schur complement of a conditional t law from the block formulas (no Cholesky factor);
  LAWS           the closed-form cases, their references, and the twin's mean on the points that the device uses.

The references of LAWS:
  (a) "one":   q = 1.  T_nuc((hi - mu) / (r sigma)) - T_nuc((lo - mu) / (r sigma)), scipy.stats.t.
  (b) "two":   q = 2 given p = 1.  scipy.integrate.dblquad of scipy.stats.multivariate_t(loc=mu, shape=r^2 Sigma, df=nu_c).pdf over
               the box: 0.35610980628 (error estimate 1e-11); multivariate_t.cdf(lower_limit=...) agrees to 1e-8 and 4e6 plain draws
               of the mixing representation give 0.35617 +- 0.00024.
               EVENT_MEANS_B: for the same case under UNIFORM marginals on (0, 1), where X_m = T_nu(Y_m), the expectations
               E[X_m | box, given] = dblquad of T_nu(y_m) pdf(y) over the box / the probability above, m = 1, 2 (error estimates
               1e-12): the deterministic value of what the mean of the conditional draws inside the event estimates.
  (c) "eye":   C = I and an extreme given value: mu = 0, Sigma = I, r > 1; one constrained component of the two others, so the
               closed form of (a) applies after the unconstrained one is dropped.  Under the Gaussian copula the conditional
               probability is the unconditional one.
"""
import numpy as np
from scipy import stats

from tests import box_prob_cases as bc
from tests import t_box_cases as tb

MIX = tb.MIX


def ct_twin(L, lo, hi, shift, scale, s, w):
    """f [n] of one box under the conditional t law: lo, hi, shift [M], scale a float, s [n] the mixing scales, w [M - 1, n]"""
    lo, hi, shift = (np.asarray(v, dtype=np.float64) for v in (lo, hi, shift))
    return tb.t_twin(L, lo - shift, hi - shift, np.float64(scale) * np.asarray(s, dtype=np.float64), w)


def scaled_limits(lo, hi, shift, scale, s):
    """((lo - shift) / c, (hi - shift) / c) [n, M] with c = scale * s [n]: the operations of the header in NumPy"""
    c = np.float64(scale) * np.asarray(s, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return (lo - shift)[None, :] / c[:, None], (hi - shift)[None, :] / c[:, None]


def problem(M, B, seed=0):
    """(L, lo, hi, shift [B, M], scale [B]): the problem of tests/t_box_cases.problem (box 1 of B > 1 has infinite upper limits, the
    last box of B = 4 an empty component) with, per box, its own nonzero shift in +-(0.05, 1) and its own scale in (0.3, 4)"""
    L, lo, hi = tb.problem(M, B, seed)
    rng = np.random.default_rng(500 + M + seed)
    shift = rng.uniform(0.05, 1.0, (B, M)) * rng.choice([-1.0, 1.0], (B, M))
    scale = rng.uniform(0.3, 4.0, B)
    return L, lo, hi, shift, scale


class Case:
    def __init__(self, M, n, first, qmc, dof, dof_mix, seeds, B):
        self.M, self.n, self.first, self.qmc, self.dof, self.dof_mix, self.seeds, self.B = M, n, first, qmc, dof, dof_mix, tuple(seeds), B
        self.L, self.lo, self.hi, self.shift, self.scale = problem(M, B)

    def __repr__(self):
        return "M{}-n{}-{}-nu{:g}-nuc{:g}-R{}-B{}".format(self.M, self.n, "sobol" if self.qmc else "philox", self.dof, self.dof_mix,
                                                          len(self.seeds), self.B)


# the shapes of tests/t_box_cases.SHAPES with nu in {1, 3, 7.5, 64}, nu_c in {nu + 1, nu + 3, 192}, R in {1, 3}, B in {1, 4}
_EXTRA = ((1.0, 2.0, (5,), 4), (3.0, 6.0, (1, 2, 3), 1), (7.5, 192.0, (4,), 4), (64.0, 65.0, (0, 9, 11), 4), (3.0, 4.0, (2,), 1),
          (7.5, 10.5, (1, 2, 3), 1), (1.0, 192.0, (6,), 4), (64.0, 67.0, (3, 4, 5), 4), (3.0, 4.0, (8,), 1))
CASES = tuple(Case(*shape, *extra) for shape, extra in zip(tb.SHAPES, _EXTRA))


# ---- the host algebra from the block formulas ---------------------------------------------------------------------------------------
def block_law(corr, observed, y_obs, dof):
    """(unobserved [q], mu [q], r, Sigma [q, q]) of the t scores of the other components given the t scores y_obs of `observed`:
    mu = C_UO C_OO^-1 y_O, r^2 = (nu + y_O^T C_OO^-1 y_O) / (nu + p), Sigma = C_UU - C_UO C_OO^-1 C_OU"""
    corr = np.asarray(corr, dtype=np.float64)
    obs = np.asarray(observed, dtype=np.int64)
    un = np.setdiff1d(np.arange(corr.shape[0]), obs)
    y = np.asarray(y_obs, dtype=np.float64).reshape(obs.size)
    coo_inv = np.linalg.inv(corr[np.ix_(obs, obs)])
    cuo = corr[np.ix_(un, obs)]
    mu = cuo @ coo_inv @ y
    r = np.sqrt((dof + y @ coo_inv @ y) / (dof + obs.size))
    return un, mu, float(r), corr[np.ix_(un, un)] - cuo @ coo_inv @ cuo.T


CORR_B = np.array([[1.0, 0.5, 0.3], [0.5, 1.0, 0.4], [0.3, 0.4, 1.0]])
DBLQUAD_B = 0.35610980628
EVENT_MEANS_B = (0.876972678382, 0.459013655196)


class Law:
    """a conditional law in t-score space: component 0 given at the t score y0; the box [lo, hi] over the other components"""

    def __init__(self, name, corr, dof, y0, lo, hi, exact):
        self.name, self.corr, self.dof, self.y0 = name, np.asarray(corr, dtype=np.float64), float(dof), float(y0)
        self.lo, self.hi, self.exact = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64), exact
        self.dof_mix = self.dof + 1.0
        _, self.mu, self.r, self.sigma = block_law(self.corr, [0], [self.y0], self.dof)
        self.keep = np.flatnonzero(np.isfinite(self.lo) | np.isfinite(self.hi))

    def __repr__(self):
        return self.name

    def reference(self):
        """the closed form of one constrained component (None where the case has a recorded reference instead)"""
        if self.keep.size != 1:
            return self.exact
        k = int(self.keep[0])
        sd_k = self.r * np.sqrt(self.sigma[k, k])
        return float(stats.t.cdf((self.hi[k] - self.mu[k]) / sd_k, self.dof_mix) - stats.t.cdf((self.lo[k] - self.mu[k]) / sd_k, self.dof_mix))

    def twin_mean(self, seeds=bc.SEEDS8, n=2 ** 12):
        """(prob, stderr) of the twin on the points of a default call: Sobol' from 0, mixing dimension 0, chain coordinate i in
        dimension i + 1; the mixing scale from SciPy's chi-square quantile (the device's differs in the last bits)"""
        k = self.keep
        low = np.linalg.cholesky(self.sigma[np.ix_(k, k)])
        means = []
        for seed in seeds:
            s = np.sqrt(self.dof_mix / stats.chi2.ppf(tb.mixing_points(seed, 0, n, True), self.dof_mix))
            w = bc.points(seed, tb.chain_streams(k.size), 0, n, True)
            means.append(ct_twin(low, self.lo[k], self.hi[k], self.mu[k], self.r, s, w).mean())
        return bc.summary(means)


LAWS = (Law("one", [[1.0, 0.6], [0.6, 1.0]], 3.0, 2.5, [-0.5], [1.5], None),
        Law("two", CORR_B, 3.0, 2.5, [0.5, -np.inf], [np.inf, 1.0], DBLQUAD_B),
        Law("eye", np.eye(3), 3.0, 6.0, [-1.0, -np.inf], [2.0, np.inf], None))
