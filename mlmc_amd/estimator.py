"""`Estimate` facade and sample-allocation helpers (reference interface: mlmc/estimator.py:11-450).

Every pass over the samples (moments, covariance, level variances) goes through
`quantity_estimate.estimate_mean`, i.e. through the HIP accumulation kernels.  The O(L R) post-processing
(variance regression over levels, n-samples allocation) is host arithmetic, as the numbers involved are tiny.
"""
import collections

import numpy as np

from . import engine
from . import linearize
from .quantity import quantity_estimate as qe
from .quantity.quantity_types import ScalarType


BootstrapReplicates = collections.namedtuple("BootstrapReplicates", "n_samples l_means l_vars mean var seed")
ComponentBootstrapReplicates = collections.namedtuple("ComponentBootstrapReplicates", "n_samples l_means l_vars mean var seed")
QuantileBands = collections.namedtuple("QuantileBands", "q lo hi replicates success n_ok seed")
ScoreCorrelation = collections.namedtuple("ScoreCorrelation", "corr cov cov_var mean var n_samples n_rm_samples")
EventMeans = collections.namedtuple("EventMeans", "mean stderr prob ess")
CovarianceBootstrapReplicates = collections.namedtuple("CovarianceBootstrapReplicates", "n_samples mean cov corr ok seed")
CorrelationBands = collections.namedtuple("CorrelationBands", "corr lo hi std replicates ok n_ok seed")
ProbabilityBands = collections.namedtuple("ProbabilityBands", "prob stderr lo hi replicates ok n_ok seed")
TailDependence = collections.namedtuple("TailDependence",
                                        "prob var chi model chi_model z marginal counts n_samples n_rm_samples corr")
JointFrequency = collections.namedtuple("JointFrequency", "prob stderr counts n_samples")
QuadrantCorrelation = collections.namedtuple("QuadrantCorrelation", "corr stderr prob var counts")
CopulaLikelihood = collections.namedtuple("CopulaLikelihood",
                                          "dof grid loglik stderr delta delta_stderr z l_means l_vars n_samples n_rm_samples corr")


def quadrant_correlation(prob, var):
    """(corr, stderr) [M, M] from the frequency prob [M, M] of two components lying above their medians at once and its variance:
    rho = sin(2 pi (P - 1/4)) clipped to [-1, 1] with a unit diagonal, stderr = 2 pi |cos(2 pi (P - 1/4))| sqrt(var), 0 on the
    diagonal (pure arithmetic, no device)"""
    prob, var = np.asarray(prob, dtype=np.float64), np.asarray(var, dtype=np.float64)
    angle = 2.0 * np.pi * (prob - 0.25)
    corr = np.clip(np.sin(angle), -1.0, 1.0)
    with np.errstate(all="ignore"):
        stderr = 2.0 * np.pi * np.abs(np.cos(angle)) * np.sqrt(var)
    np.fill_diagonal(corr, 1.0)
    np.fill_diagonal(stderr, 0.0)
    return corr, stderr


def covariance_replicates(n, s1, s2, sample_vector, shift=None, centered=True):
    """Host finish of the component-covariance bootstrap (pure arithmetic, no device): n [B, L] kept counts, s1 [B, L, M] and
    s2 [B, L, M, M] the per-replicate level sums of the shifted first moments and products
    (quantity_estimate.bootstrap_component_covariance), sample_vector [L] the requested samples per level, shift a [M] | None.
    Over the levels with sample_vector[l] > 0:  m_b = sum_l s1 / n,  S_b = sum_l s2 / n,  mean_b = m_b + a,
    cov_b = S_b - m_b m_b^T (every replicate centred on its OWN mean; symmetrised), corr_b = cov_b / (sd sd^T) with a unit
    diagonal.  centered=False: `cov` holds the raw second moments S_b instead (corr is still that of S_b - m_b m_b^T).
    ok[b] is False when a level with sample_vector[l] > 0 has n = 0 or a variance is not positive and finite; the rows of such a
    replicate are NaN.  -> (mean [B, M], cov [B, M, M], corr [B, M, M], ok [B])"""
    n = np.asarray(n)
    s1 = np.asarray(s1, dtype=np.float64)
    s2 = np.asarray(s2, dtype=np.float64)
    if n.ndim != 2 or s1.shape[:2] != n.shape or s2.shape != s1.shape + s1.shape[2:]:
        raise ValueError("covariance_replicates: n [B, L], s1 [B, L, M] and s2 [B, L, M, M] expected, got shapes {}, {} and {}".format(
            n.shape, s1.shape, s2.shape))
    B, L, M = s1.shape
    used = np.asarray(sample_vector).reshape(-1) > 0
    if used.shape != (L,):
        raise ValueError("covariance_replicates: sample_vector must hold one value per level ({}), got {!r}".format(L, sample_vector))
    a = np.zeros(M) if shift is None else np.asarray(shift, dtype=np.float64).reshape(M)
    nf = n[:, used].astype(np.float64)
    ok = np.all(nf > 0, axis=1)
    with np.errstate(all="ignore"):
        m = np.sum(s1[:, used] / nf[:, :, None], axis=1)
        S = np.sum(s2[:, used] / nf[:, :, None, None], axis=1)
        cov = S - m[:, :, None] * m[:, None, :]
        cov = 0.5 * (cov + cov.transpose(0, 2, 1))
        var = np.diagonal(cov, axis1=1, axis2=2)
        ok = ok & np.all(np.isfinite(var) & (var > 0), axis=1)
        sd = np.sqrt(var)
        corr = cov / (sd[:, :, None] * sd[:, None, :])
    idx = np.arange(M)
    corr[:, idx, idx] = 1.0
    mean = m + a[None, :]
    out_cov = cov if centered else 0.5 * (S + S.transpose(0, 2, 1))
    mean[~ok] = np.nan
    out_cov[~ok] = np.nan
    corr[~ok] = np.nan
    return mean, out_cov, corr, ok


def _band_over_ok(replicates, ok, level):
    """quantile_bands of replicates [B, ...] over the ok replicates -> (lo, hi) of the trailing shape"""
    replicates = np.asarray(replicates, dtype=np.float64)
    flat = replicates.reshape(replicates.shape[0], 1, -1)
    lo, hi = quantile_bands(flat, np.asarray(ok, dtype=bool)[:, None], level)
    return lo.reshape(replicates.shape[1:]), hi.reshape(replicates.shape[1:])


def quantile_bands(replicates, success, level):
    """Percentile bands of bootstrap quantile replicates (host arithmetic): replicates [B, M, P], success [B, M] bool ->
    (lo, hi) [M, P], the 100 (1 - level) / 2 and 100 (1 + level) / 2 percentiles (np.percentile, axis 0) of component m's
    replicates over its successful rows alone; NaN for a component without a successful replicate."""
    replicates = np.asarray(replicates, dtype=np.float64)
    success = np.asarray(success, dtype=bool)
    if replicates.ndim != 3 or success.shape != replicates.shape[:2]:
        raise ValueError("quantile_bands: replicates [B, M, P] and success [B, M] expected, got shapes {} and {}".format(
            replicates.shape, success.shape))
    level = _check_level("quantile_bands", level)
    _, M, P = replicates.shape
    lo = np.full((M, P), np.nan)
    hi = np.full((M, P), np.nan)
    for m in range(M):
        rows = replicates[success[:, m], m]
        if rows.shape[0]:
            lo[m] = np.percentile(rows, 100.0 * (1.0 - level) / 2.0, axis=0)
            hi[m] = np.percentile(rows, 100.0 * (1.0 + level) / 2.0, axis=0)
    return lo, hi


DivergenceSpread = collections.namedtuple("DivergenceSpread", "kl l2 tv hellinger upper success n_ok seed")


def divergence_upper(measures, success, level):
    """One-sided percentile of bootstrap divergence replicates (host arithmetic): measures = four [B, M] arrays (kl, l2, tv,
    hellinger), success [B, M] bool -> upper [M, 4], the 100 level percentile (np.percentile) of each measure over component m's
    successful replicates alone, in that column order; NaN for a component without a successful replicate.  One-sided because
    the measures are non-negative: their spread has 0 as its natural lower end."""
    stack = np.stack([np.asarray(v, dtype=np.float64) for v in measures], axis=-1)
    success = np.asarray(success, dtype=bool)
    if stack.ndim != 3 or stack.shape[2] != 4 or success.shape != stack.shape[:2]:
        raise ValueError("divergence_upper: four measures [B, M] and success [B, M] expected, got shapes {} and {}".format(
            stack.shape, success.shape))
    level = _check_level("divergence_upper", level)
    M = stack.shape[1]
    upper = np.full((M, 4), np.nan)
    for m in range(M):
        rows = stack[success[:, m], m]
        if rows.shape[0]:
            upper[m] = np.percentile(rows, 100.0 * level, axis=0)
    return upper


def _check_level(what, level):
    if isinstance(level, (bool, np.bool_)) or not isinstance(level, (int, float, np.integer, np.floating)) or not 0.0 < level < 1.0:
        raise ValueError("{}: level must be a number in (0, 1), got {!r}".format(what, level))
    return float(level)


AggregateSummary = collections.namedtuple(
    "AggregateSummary", "names probs quantiles quantiles_stderr mean mean_stderr var var_stderr shortfall shortfall_stderr count_prob "
    "count_prob_stderr worst_prob worst_prob_stderr best_prob best_prob_stderr prob n seeds")


def _weighted_row_quantiles(rows, f, probs):
    """[Q, K]: the weighted quantiles of every row under the weights f by the rule of EventScenarios.weighted_quantiles: the smallest
    value at which the cumulated normalised weight reaches p.  NaN for a row that holds a NaN or when the weights sum to nothing"""
    out = np.full((rows.shape[0], probs.size), np.nan)
    total = f.sum()
    if not total > 0:
        return out
    for k, x in enumerate(rows):
        if np.any(np.isnan(x)):
            continue
        order = np.argsort(x, kind="stable")
        cum = np.cumsum(f[order]) / total
        out[k] = x[order][np.minimum(np.searchsorted(cum, probs, side="left"), x.size - 1)]
    return out


def _check_tail(what, tail):
    if tail not in ("upper", "lower"):
        raise ValueError("{}: tail must be 'upper' or 'lower', got {!r}".format(what, tail))


def _refuse_dof_with_given(what, dof, given):
    """estimate_aggregates conditions under the Gaussian copula only"""
    if dof is not None and given is not None:
        raise ValueError(what + ": dof together with given: this method conditions under the Gaussian copula only; call "
                         "estimate_conditional_aggregates")


def _conditional_dof_with_given(what, dof, given):
    """the conditional family: dof + the number of given components must stay within 192"""
    from .tool import simple_distribution
    simple_distribution._check_conditional_dof(what, dof, len(given) if hasattr(given, "items") else 0)


class Estimate:
    """Wrapper methods for moment estimation, sample allocation and PDF reconstruction (reference: estimator.py:11-341)."""

    def __init__(self, quantity, sample_storage, moments_fn=None):
        self._quantity = quantity
        self._sample_storage = sample_storage
        self._moments_fn = moments_fn

    @property
    def quantity(self):
        return self._quantity

    @quantity.setter
    def quantity(self, quantity):
        self._quantity = quantity

    @property
    def n_moments(self):
        return self._moments_fn.size

    # ---- estimates (device passes) -------------------------------------------------------------------
    def estimate_moments(self, moments_fn=None):
        """-> (moment means, variances of these estimates), arrays of length n_moments (reference: :32-42)."""
        if moments_fn is None:
            moments_fn = self._moments_fn
        r = qe.estimate_mean(qe.moments(self._quantity, moments_fn))
        return r.mean, r.var

    def estimate_covariance(self, moments_fn=None):
        """-> (covariance matrix of the moments, variance of its entries) (reference: :44-54)."""
        if moments_fn is None:
            moments_fn = self._moments_fn
        r = qe.estimate_mean(qe.covariance(self._quantity, moments_fn))
        self._cov_memo = (self._memo_key(moments_fn), r, moments_fn, self._quantity)
        return r.mean, r.var

    def estimate_component_covariance(self, centered=True):
        """-> (cov [M, M], cov_var [M, M]): the multilevel covariance between the M scalar components of the quantity (row order
        as construct_densities documents) and the variance of each entry's estimate (sum over levels of l_vars / n_l).

        centered=True: the shift a is the MLMC mean of the quantity (estimate_mean(quantity), a first pass), and cov is the
        plug-in estimator E[(Q - mu^)(Q - mu^)^T] = sum_l mean_l((f - a)(f - a)^T - (c - a)(c - a)^T) with a = mu^; the shift
        also spares the sums the cancellation of raw second moments when |mean| >> std.  It is the plug-in form: the
        unbiased multilevel covariance with per-level sample covariances and n / (n - 1) corrections is not provided.
        centered=False: raw second moments E[Q Q^T] (a = 0), entry (i, j) = estimate_mean(q_i * q_j).mean.
        One pass of the component-covariance kernel per stored chunk (quantity_estimate.component_covariance)."""
        M = int(self._quantity.size())
        shift = None
        if centered:
            shift = np.asarray(qe.estimate_mean(self._quantity).mean, dtype=np.float64).reshape(M)
        r = qe.estimate_mean(qe.component_covariance(self._quantity, shift))
        return np.asarray(r.mean).reshape(M, M), np.asarray(r.var).reshape(M, M)

    def _memo_key(self, moments_fn):
        """What a kept covariance estimate is valid for: this quantity object, these moment functions, the stamps of the
        storage's levels (samples collected + modification counts, quantity_estimate._level_stamps)."""
        try:
            stamps = qe._level_stamps(self._quantity.get_quantity_storage())
        except Exception:
            return None
        return (stamps, qe.device_cache_generation())

    def _diff_vars_from_covariance(self, moments_fn):
        """Level sums of the moments out of the last covariance estimate of the same (quantity, moments_fn, samples):
        row 0 of the covariance rows is phi_0 phi_j = phi_j, so its level means / variances ARE those of the moments
        (engine.moments_from_covariance) -- no second pass over the samples.  None when no such estimate is at hand."""
        memo = getattr(self, "_cov_memo", None)
        # the memo holds the quantity and the moment functions themselves (compared with `is`: an id() can be reused)
        if memo is None or memo[0] is None or memo[0] != self._memo_key(moments_fn) or memo[2] is not moments_fn \
                or memo[3] is not self._quantity:
            return None
        from .moments import Legendre, Monomial, Fourier, Spline
        if type(moments_fn) not in (Legendre, Monomial, Fourier, Spline):
            return None          # only the families known to start with the constant: phi_0 = 1 (moments.py:122-126,145-162,195-197)
        r, size = memo[1], moments_fn.size
        n_levels = r._l_means.shape[0]
        n_comp = r._l_means.shape[1] // (size * size)
        l_means, l_vars = engine.moments_from_covariance(r._l_means, r._l_vars, size, n_comp=n_comp)
        from .quantity.quantity import QuantityMean
        return QuantityMean(qe.moments(self._quantity, moments_fn).qtype, l_means=l_means.reshape(n_levels, -1),
                            l_vars=l_vars.reshape(n_levels, -1), n_samples=r.n_samples, n_rm_samples=r.n_rm_samples)

    def estimate_diff_vars(self, moments_fn=None):
        """-> (variances of the level differences [L, R], n_samples [L]) (reference: :76-85).  After estimate_covariance
        of the same moment functions on unchanged samples the variances are read from the covariance estimate."""
        if moments_fn is None:
            moments_fn = self._moments_fn
        r = self._diff_vars_from_covariance(moments_fn)
        if r is None:
            r = qe.estimate_mean(qe.moments(self._quantity, moments_fn))
        return r.l_vars, r.n_samples

    def estimate_diff_vars_regression(self, n_created_samples, moments_fn=None, raw_vars=None):
        """Level variances smoothed by a log-quadratic model in the level step (reference: :56-74).
        -> (vars [L, R], n_ops [L])"""
        self._n_created_samples = n_created_samples
        if raw_vars is None:
            if moments_fn is None:
                moments_fn = self._moments_fn
            raw_vars, _ = self.estimate_diff_vars(moments_fn)
        sim_steps = np.squeeze(self._sample_storage.get_level_parameters())
        return self._all_moments_variance_regression(raw_vars, sim_steps), self._sample_storage.get_n_ops()

    # ---- per-component estimates of a vector quantity -----------------------------------------------------------------
    def _component_fns(self, moments_fns, what):
        """moments_fns checked before any device work: M objects of one size (None: this Estimate's moments_fn for all)."""
        n_comp = int(self._quantity.size())
        if moments_fns is None:
            if self._moments_fn is None:
                raise ValueError("{}: no moments_fn given and none set on this Estimate".format(what))
            moments_fns = [self._moments_fn] * n_comp
        moments_fns = list(moments_fns)
        if len(moments_fns) != n_comp:
            raise ValueError("{}: {} moments objects for {} components".format(what, len(moments_fns), n_comp))
        sizes = sorted({int(fn.size) for fn in moments_fns})
        if len(sizes) != 1:
            raise ValueError("{}: the moments objects must all have the same size, got sizes {}".format(what, sizes))
        return moments_fns

    def _component_estimate(self, moments_fns):
        """-> n [L, M] int64, l_vars [L, M, R], mean [M, R], var [M, R]: row m is the scalar estimate_mean(moments(q_m, fn_m)).
        Legendre / monomial / Fourier moments of one family: ONE device pass per stored chunk for all components
        (quantity_estimate.component_level_sums); other moments: the per-component loop of scalar estimates."""
        if qe.component_device_route(moments_fns):
            n, _, s, sp = qe.component_level_sums(self._quantity, moments_fns)
            _, l_vars, mean, var = qe.component_statistics(n, s, sp)
            return n, l_vars, mean, var
        comps = [self._quantity] if isinstance(self._quantity.qtype, ScalarType) else \
            [scalar_component(self._quantity, m) for m in range(len(moments_fns))]
        rs = qe.component_estimates(comps, moments_fns)
        R = int(moments_fns[0].size)
        n = np.stack([np.asarray(r.n_samples, dtype=np.int64) for r in rs], axis=1)
        l_vars = np.stack([np.asarray(r.l_vars).reshape(-1, R) for r in rs], axis=1)
        mean = np.stack([np.asarray(r.mean).reshape(R) for r in rs])
        var = np.stack([np.asarray(r.var).reshape(R) for r in rs])
        return n, l_vars, mean, var

    def estimate_component_moments(self, moments_fns=None):
        """-> (means [M, R], vars [M, R]): row m is Estimate(q_m, storage, fn_m).estimate_moments() for the scalar component
        q_m = scalar_component(quantity, m) (row order as construct_densities documents), each component masked and clipped on
        its own.  moments_fns: M moments objects of one size R (None: this Estimate's moments_fn for every component)."""
        fns = self._component_fns(moments_fns, "estimate_component_moments")
        _, _, mean, var = self._component_estimate(fns)
        return mean, var

    def estimate_component_diff_vars(self, moments_fns=None):
        """-> (l_vars [L, M, R], n_samples [L, M] int64): column m is Estimate(q_m, storage, fn_m).estimate_diff_vars()."""
        fns = self._component_fns(moments_fns, "estimate_component_diff_vars")
        n, l_vars, _, _ = self._component_estimate(fns)
        return l_vars, n

    def estimate_component_diff_vars_regression(self, n_created_samples, moments_fns=None, raw_vars=None):
        """-> (vars [L, M, R], n_ops [L]): estimate_diff_vars_regression of every component, the regression of
        _all_moments_variance_regression over the [L, M * R] level variances (the columns of phi_0 are zero and left alone).
        For the sample allocation: estimate_n_samples_for_target_variance(target, vars.reshape(L, -1), n_ops, L).
        raw_vars: [L, M, R] level variances to regress instead of estimating them."""
        self._n_created_samples = n_created_samples
        if raw_vars is None:
            raw_vars, _ = self.estimate_component_diff_vars(moments_fns)
        raw_vars = np.asarray(raw_vars, dtype=np.float64)
        if raw_vars.ndim != 3:
            raise ValueError("estimate_component_diff_vars_regression: raw_vars must be [L, M, R], got shape {}".format(
                raw_vars.shape))
        n_levels = raw_vars.shape[0]
        sim_steps = np.squeeze(self._sample_storage.get_level_parameters())
        reg = self._all_moments_variance_regression(raw_vars.reshape(n_levels, -1), sim_steps).reshape(raw_vars.shape)
        return reg, self._sample_storage.get_n_ops()

    def estimate_level_diagnostics(self):
        """-> diagnostics.LevelDiagnostics: the MLMC convergence tests of the level hierarchy for EVERY scalar component of the
        quantity (any qtype, scalar included; row order as construct_densities documents; no moments function needed), [L, M]
        arrays: kurtosis and skewness of the level differences, mean and variance of the differences, of the fine and of the
        coarse values, the fine / coarse correlation, the telescoping-consistency check between neighbouring levels, and
        through `.rates()` / `.flags()` the decay rates alpha, beta, gamma and the levels that fail the checks.  Each
        component is NaN-masked on its own.  Two device passes per stored chunk for all components
        (quantity_estimate.level_diagnostics)."""
        from . import diagnostics
        n, _, stats = qe.level_diagnostics(self._quantity)
        level_steps = np.squeeze(self._sample_storage.get_level_parameters())
        n_ops = self._sample_storage.get_n_ops()
        if n_ops is None or len(n_ops) != n.shape[0]:
            n_ops = None                                   # the storage has no costs (for every level): gamma is NaN
        return diagnostics.from_central_sums(n, stats, level_steps=level_steps, n_ops=n_ops)

    def _all_moments_variance_regression(self, raw_vars, sim_steps):
        """Per-moment regression of the level variances (reference: :87-93), all moments in ONE least-squares solve with
        several right-hand sides (the design matrix [1, log h, log^2 h] is the same for every moment)."""
        raw_vars = np.asarray(raw_vars, dtype=np.float64)
        reg_vars = np.array(raw_vars, copy=True)
        n_levels = raw_vars.shape[0]
        if n_levels >= 3:
            # moments whose level variances are all (close to) zero are left alone, as np.allclose(raw_vars[:, m], 0) decides it
            cols = 1 + np.flatnonzero(~np.all(np.isclose(raw_vars[:, 1:], 0), axis=0))
            if cols.size:
                log_h = np.log(np.asarray(sim_steps, dtype=np.float64)[1:])
                design = np.stack([np.ones(n_levels - 1), log_h, log_h ** 2], axis=1)
                with np.errstate(all="ignore"):
                    params = np.linalg.lstsq(design, np.log(raw_vars[1:][:, cols]), rcond=None)[0]
                    reg_vars[1:, cols] = np.exp(design @ params)
        assert np.allclose(reg_vars[:, 0], 0.0)
        return reg_vars

    def _moment_variance_regression(self, raw_vars, sim_steps):
        """log var_l = A + B log h_l + C log^2 h_l fitted on levels 1..L-1, unweighted; level 0 is kept
        (reference: :95-134 -- its chi-square weights are computed and then overwritten by ones, :111-113)."""
        raw_vars = np.asarray(raw_vars, dtype=np.float64)
        n_levels = raw_vars.shape[0]
        if n_levels < 3 or np.allclose(raw_vars, 0):
            return raw_vars
        log_h = np.log(np.asarray(sim_steps, dtype=np.float64)[1:])
        design = np.stack([np.ones(n_levels - 1), log_h, log_h ** 2], axis=1)
        params = np.linalg.lstsq(design, np.log(raw_vars[1:]), rcond=None)[0]
        fitted = raw_vars.copy()
        fitted[1:] = np.exp(design @ params)
        return fitted

    def _variance_of_variance(self, n_samples=None):
        """Variance of log(chi^2_{n-1} / (n-1)) per level (reference: :136-169).  Closed form instead of the reference's
        two adaptive quadratures per level: Var[log X], X ~ chi2_df / df, equals trigamma(df / 2)."""
        from scipy.special import polygamma
        if n_samples is None:
            n_samples = self._n_created_samples
        return np.array([float(polygamma(1, (ns - 1) / 2.0)) for ns in n_samples])

    # ---- bootstrap ------------------------------------------------------------------------------------
    def est_bootstrap(self, n_subsamples=100, sample_vector=None, moments_fn=None):
        """Bootstrap statistics of the estimates over random sub-samples (reference: :171-205)."""
        if moments_fn is not None:
            self._moments_fn = moments_fn
        else:
            moments_fn = self._moments_fn
        sample_vector = determine_sample_vec(n_collected_samples=self._sample_storage.get_n_collected(),
                                             n_levels=self._sample_storage.get_n_levels(), sample_vector=sample_vector)
        bs_mean, bs_var, bs_l_means, bs_l_vars = [], [], [], []
        for _ in range(n_subsamples):
            # The reference writes quantity.select(quantity.subsample(...)) here (estimator.py:186), which indexes the
            # chunk with the picked *values* and raises IndexError; its own test (test_quantity_concept.py:630-648) uses
            # the sub-sampled quantity directly, as done here.
            sub = self.quantity.subsample(sample_vec=sample_vector)
            q_mean = qe.estimate_mean(qe.moments(sub, moments_fn=moments_fn, mom_at_bottom=False))
            bs_mean.append(q_mean.mean)
            bs_var.append(q_mean.var)
            bs_l_means.append(q_mean.l_means)
            bs_l_vars.append(q_mean.l_vars)
        self.mean_bs_mean = np.mean(bs_mean, axis=0)
        self.mean_bs_var = np.mean(bs_var, axis=0)
        self.mean_bs_l_means = np.mean(bs_l_means, axis=0)
        self.mean_bs_l_vars = np.mean(bs_l_vars, axis=0)
        self.var_bs_mean = np.var(bs_mean, axis=0, ddof=1)
        self.var_bs_var = np.var(bs_var, axis=0, ddof=1)
        self.var_bs_l_means = np.var(bs_l_means, axis=0, ddof=1)
        self.var_bs_l_vars = np.var(bs_l_vars, axis=0, ddof=1)
        n_coll = np.array(self._sample_storage.get_n_collected())
        # [L, R] for scalar quantities (reference: `[:, None]`); array-typed quantities carry extra trailing axes
        self._bs_level_mean_variance = self.var_bs_l_means * n_coll.reshape((-1,) + (1,) * (self.var_bs_l_means.ndim - 1))

    def est_bootstrap_batch(self, n_subsamples=100, sample_vector=None, moments_fn=None, seed=None):
        """est_bootstrap with every replicate from one device pass per stored chunk, seeded.

        Replicate b draws, in stored chunk c of level l (n_c samples, N_l collected, k_l = sample_vector[l] requested), a
        Hypergeometric(k_l, N_l - k_l, min(n_c, N_l)) count s from a generator keyed by (seed, l, c), then s of the chunk's samples
        uniformly with replacement (Philox, keyed by the seed) -- the distribution of est_bootstrap's sub-samples.  Its results are
        those of estimate_mean(moments(q, fn, mom_at_bottom=False)) over that resample; the moments of each stored sample are
        evaluated once, the replicates are an integer-weighted contraction on the matrix cores (mlmc_bootstrap_accum).  Results are
        bit-identical from run to run, and the first B replicates do not depend on n_subsamples.  Sets the attributes of
        est_bootstrap (mean_bs_* / var_bs_* over the replicates, _bs_level_mean_variance).
        :param seed: None: one 63-bit seed drawn from quantity.RNG (seeding that RNG makes the call reproducible)
        :return: BootstrapReplicates(n_samples [B, L], l_means, l_vars, mean, var -- leading axis B -- and the seed)
        Legendre, monomial and Fourier moments only (log / safe_eval included); est_bootstrap serves the others."""
        from .moments import Legendre, Monomial, Fourier
        if moments_fn is None:
            moments_fn = self._moments_fn
        if type(moments_fn) not in (Legendre, Monomial, Fourier):
            raise ValueError("est_bootstrap_batch: {} moments are not supported (Legendre, Monomial and Fourier are); use "
                             "est_bootstrap for them".format(type(moments_fn).__name__))
        if int(self._quantity.size()) * moments_fn.size > 2048:
            raise ValueError("est_bootstrap_batch: {} components x {} moments, at most 2048 columns are supported".format(
                int(self._quantity.size()), moments_fn.size))
        n_subsamples, k, seed = self._bootstrap_args("est_bootstrap_batch", n_subsamples, sample_vector, seed)
        n_coll = np.array(self._sample_storage.get_n_collected())[:len(k)]
        self._moments_fn = moments_fn
        n, s, sp = qe.bootstrap_moments(self._quantity, moments_fn, n_subsamples, k, seed)
        r = qe.bootstrap_statistics(self._quantity, moments_fn, n, s, sp)
        self.mean_bs_mean = np.mean(r["mean"], axis=0)
        self.mean_bs_var = np.mean(r["var"], axis=0)
        self.mean_bs_l_means = np.mean(r["l_means"], axis=0)
        self.mean_bs_l_vars = np.mean(r["l_vars"], axis=0)
        self.var_bs_mean = np.var(r["mean"], axis=0, ddof=1)
        self.var_bs_var = np.var(r["var"], axis=0, ddof=1)
        self.var_bs_l_means = np.var(r["l_means"], axis=0, ddof=1)
        self.var_bs_l_vars = np.var(r["l_vars"], axis=0, ddof=1)
        self._bs_level_mean_variance = self.var_bs_l_means * n_coll.reshape((-1,) + (1,) * (self.var_bs_l_means.ndim - 1))
        return BootstrapReplicates(r["n_samples"], r["l_means"], r["l_vars"], r["mean"], r["var"], seed)

    def _bootstrap_args(self, what, n_subsamples, sample_vector, seed):
        """The replicate count, the requested samples per level and the seed of a batched bootstrap (`what`: the caller's name),
        checked before any device work.  -> (B, k [L] int64, seed)"""
        from .quantity import quantity as qmod
        if isinstance(n_subsamples, (bool, np.bool_)) or not isinstance(n_subsamples, (int, np.integer)) or n_subsamples < 1:
            raise ValueError("{}: n_subsamples must be an integer >= 1, got {!r}".format(what, n_subsamples))
        n_levels = self._sample_storage.get_n_levels()
        n_coll = np.array(self._sample_storage.get_n_collected())[:n_levels]
        k = determine_sample_vec(n_collected_samples=n_coll, n_levels=n_levels, sample_vector=sample_vector)
        if k.shape != (n_levels,) or k.dtype.kind not in "iuf" or not np.all(np.isfinite(k.astype(np.float64))) or \
                np.any(k != np.round(k)):
            raise ValueError("{}: sample_vector must hold one integer per level, got {!r}".format(what, sample_vector))
        k = k.astype(np.int64)
        if np.any(k < 0) or np.any(k > n_coll):
            raise ValueError("{}: sample_vector {} must lie in 0 .. n_collected {} on every level".format(
                what, k.tolist(), n_coll.tolist()))
        if seed is None:
            seed = int(qmod.RNG.integers(0, 2 ** 63 - 1))
        if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
            raise ValueError("{}: seed must be an integer in [0, 2^64), got {!r}".format(what, seed))
        return int(n_subsamples), k, int(seed)

    def _component_bootstrap_args(self, what, n_subsamples, sample_vector, moments_fns, seed):
        """The arguments of the per-component bootstrap, checked before any device work.
        -> (moments objects [M], B, k [L] int64, seed)"""
        fns = self._component_fns(moments_fns, what)
        from .moments import Legendre, Monomial, Fourier
        names = sorted({type(fn).__name__ for fn in fns})
        if len(names) != 1 or type(fns[0]) not in (Legendre, Monomial, Fourier):
            raise ValueError("{}: {} moments are not supported (Legendre, Monomial or Fourier objects of ONE family are); use "
                             "est_bootstrap or est_bootstrap_batch on scalar_component(quantity, m) for them".format(
                                 what, " / ".join(names)))
        if int(fns[0].size) > 512:
            raise ValueError("{}: {} moments per component, at most 512 are supported".format(what, int(fns[0].size)))
        return (fns,) + self._bootstrap_args(what, n_subsamples, sample_vector, seed)

    def est_bootstrap_components(self, n_subsamples=100, sample_vector=None, moments_fns=None, seed=None):
        """est_bootstrap_batch of EVERY scalar component of the quantity under its own moments object, from one device pass per
        stored chunk for all components (mlmc_bootstrap_create_multi).

        Slice [:, ..., m, :] of every result is what `Estimate(scalar_component(q, m), storage, moments_fns[m])
        .est_bootstrap_batch(n_subsamples, sample_vector, seed=seed)` returns: component m has its own domain and is NaN-masked and
        clipped on its own (a NaN in component 3 does not touch component 0 -- est_bootstrap_batch on the vector quantity drops
        the sample for all), and replicate b is drawn with the very weights of the scalar call.  No column limit; Legendre,
        Monomial and Fourier objects of one family and size.  Bit-identical from run to run, the first B replicates do not
        depend on n_subsamples.  A level with sample_vector[l] = 0 gives NaN means and inf variances, as est_bootstrap_batch.
        :param moments_fns: M moments objects (None: this Estimate's moments_fn for every component)
        :param seed: None: one 63-bit seed drawn from quantity.RNG
        :return: ComponentBootstrapReplicates(n_samples [B, L, M], l_means [B, L, M, R], l_vars [B, L, M, R], mean [B, M, R],
            var [B, M, R], seed); a scalar quantity has M = 1"""
        fns, B, k, seed = self._component_bootstrap_args("est_bootstrap_components", n_subsamples, sample_vector, moments_fns, seed)
        n, s, sp = qe.bootstrap_component_moments(self._quantity, fns, B, k, seed)
        if np.any(np.sum(n, axis=1) == 0):
            raise Exception("All samples were masked")
        _, L, M, R = s.shape
        l_means, l_vars = engine.level_stats(n.reshape(-1), s.reshape(-1, R), sp.reshape(-1, R))
        l_means, l_vars = l_means.reshape(B, L, M, R), l_vars.reshape(B, L, M, R)
        mean = np.sum(l_means, axis=1)
        with np.errstate(all="ignore"):
            var = np.sum(l_vars / n[..., None], axis=1)
        return ComponentBootstrapReplicates(n, l_means, l_vars, mean, var, seed)

    def bootstrap_component_quantiles(self, probs, n_subsamples=100, sample_vector=None, seed=None, level=0.9, tol=1e-8,
                                      reg_param=0.0, orth_moments_tol=1e-4, moments_fns=None, densities=None):
        """Bootstrap confidence bands of estimate_component_quantiles: how far the quantiles of every component's maximum-entropy
        density move under resampling of the stored samples.

        The orthogonal moments object of every component (matrix T_m, domain) is the one of `densities` (construct_densities,
        computed here if not given) and stays fixed.  One est_bootstrap_components pass gives the level sums of the base moments of
        every (replicate, component); replicate moments are mu_bm = sum_l (s[b, l, m] / n[b, l, m]) @ T_m^T over the levels with
        sample_vector[l] > 0 (the arithmetic of construct_densities); the B * M max-entropy problems are solved in ONE batched
        device call and their quantiles taken in ONE more.  A replicate equals the single solve of the same moments bit for bit
        (tool.simple_distribution.quantiles).
        :param probs: probabilities, the same for every component
        :param level: coverage of the band, 0 < level < 1 (0.9: the 5 % .. 95 % percentiles over the replicates)
        :param moments_fns: base moments objects of the bootstrap pass (None: those of `densities`)
        :return: QuantileBands(q [M, P] = estimate_component_quantiles(probs, densities=densities)[0], lo [M, P], hi [M, P] =
            quantile_bands(replicates, success, level), replicates [B, M, P], success [B, M] the solver's verdict per replicate,
            n_ok [M] successful replicates per component, seed)"""
        from .tool import simple_distribution
        probs, densities, distrs, success, seed, level = self._bootstrap_replicate_densities(
            "bootstrap_component_quantiles", probs, n_subsamples, sample_vector, seed, level, tol, reg_param, orth_moments_tol,
            moments_fns, densities)
        q = self.estimate_component_quantiles(probs, densities=densities)[0]
        replicates = np.array(simple_distribution.quantiles(distrs, probs), dtype=np.float64).reshape(success.shape + (probs.size,))
        lo, hi = quantile_bands(replicates, success, level)
        return QuantileBands(q, lo, hi, replicates, success, np.sum(success, axis=0), seed)

    def bootstrap_component_shortfall(self, probs, n_subsamples=100, sample_vector=None, seed=None, level=0.9, tail="upper", tol=1e-8,
                                      reg_param=0.0, orth_moments_tol=1e-4, moments_fns=None, densities=None):
        """Bootstrap confidence bands of estimate_component_shortfall: bootstrap_component_quantiles with the expected shortfall
        (tool.simple_distribution.tail_means) of every replicate density in place of its quantiles.  Same arguments, the same
        replicate densities for the same seed, and
        :param tail: "upper" (E[X | X >= Q(p)]) or "lower" (E[X | X <= Q(p)])
        :return: QuantileBands whose q [M, P] = estimate_component_shortfall(probs, tail, densities=densities)[0], lo, hi [M, P]
            and replicates [B, M, P] hold the shortfall values; success, n_ok, seed as in bootstrap_component_quantiles"""
        from .tool import simple_distribution
        what = "bootstrap_component_shortfall"
        _check_tail(what, tail)
        probs, densities, distrs, success, seed, level = self._bootstrap_replicate_densities(
            what, probs, n_subsamples, sample_vector, seed, level, tol, reg_param, orth_moments_tol, moments_fns, densities)
        es = self.estimate_component_shortfall(probs, tail, densities=densities)[0]
        _, lower, upper, _ = simple_distribution.tail_means(distrs, probs)
        replicates = np.array(upper if tail == "upper" else lower, dtype=np.float64).reshape(success.shape + (probs.size,))
        lo, hi = quantile_bands(replicates, success, level)
        return QuantileBands(es, lo, hi, replicates, success, np.sum(success, axis=0), seed)

    def bootstrap_component_divergences(self, n_subsamples=100, sample_vector=None, seed=None, level=0.9, tol=1e-8, reg_param=0.0,
                                        orth_moments_tol=1e-4, moments_fns=None, densities=None):
        """How far the maximum-entropy density of every component itself moves under resampling of the stored samples: the
        divergences (tool.simple_distribution.divergences) of every bootstrap replicate density (the posterior) from the
        component's estimated density (the prior) on the component's domain, all B * M pairs in ONE device call.  Same arguments
        and, for the same seed, the same replicate densities as bootstrap_component_quantiles.
        :param level: 0 < level < 1, the percentile of `upper`
        :return: DivergenceSpread(kl, l2, tv, hellinger [B, M], upper [M, 4] = divergence_upper((kl, l2, tv, hellinger), success,
            level), success [B, M] the solver's verdict per replicate, n_ok [M], seed)"""
        from .tool import simple_distribution
        _, densities, distrs, success, seed, level = self._bootstrap_replicate_densities(
            "bootstrap_component_divergences", None, n_subsamples, sample_vector, seed, level, tol, reg_param, orth_moments_tol,
            moments_fns, densities)
        B, M = success.shape
        res = simple_distribution.divergences([densities[m][0] for _ in range(B) for m in range(M)], distrs)
        measures = [np.asarray(v, dtype=np.float64).reshape(B, M) for v in (res.kl, res.l2, res.tv, res.hellinger)]
        return DivergenceSpread(*measures, divergence_upper(measures, success, level), success, np.sum(success, axis=0), seed)

    def bootstrap_component_summaries(self, n_subsamples=100, sample_vector=None, seed=None, level=0.9, tol=1e-8, reg_param=0.0,
                                      orth_moments_tol=1e-4, moments_fns=None, densities=None):
        """Bootstrap confidence bands of estimate_component_summaries: bootstrap_component_quantiles with the statistics of every
        replicate density (tool.simple_distribution.summaries) in place of its quantiles.  Same arguments and, for the same seed,
        the same replicate densities.
        :return: QuantileBands whose five columns are mean, var, skewness, kurtosis and entropy: q [M, 5] = the statistics of
            estimate_component_summaries(densities=densities), lo, hi [M, 5] = quantile_bands(replicates, success, level),
            replicates [B, M, 5]; success, n_ok, seed as in bootstrap_component_quantiles"""
        from .tool import simple_distribution
        _, densities, distrs, success, seed, level = self._bootstrap_replicate_densities(
            "bootstrap_component_summaries", None, n_subsamples, sample_vector, seed, level, tol, reg_param, orth_moments_tol,
            moments_fns, densities)
        q = np.stack(self.estimate_component_summaries(densities=densities)[:5], axis=1)
        replicates = np.stack(simple_distribution.summaries(distrs)[:5], axis=1).reshape(success.shape + (5,))
        lo, hi = quantile_bands(replicates, success, level)
        return QuantileBands(q, lo, hi, replicates, success, np.sum(success, axis=0), seed)

    def _bootstrap_replicate_densities(self, what, probs, n_subsamples, sample_vector, seed, level, tol, reg_param, orth_moments_tol,
                                       moments_fns, densities):
        """The part bootstrap_component_quantiles and bootstrap_component_shortfall share: argument checks, the densities of the
        estimate, one est_bootstrap_components pass and the B * M replicate max-entropy problems solved in one batched call.
        :return: (probs [P], densities, distrs [B * M] solved replicate distributions (replicate-major), success [B, M], seed, level)"""
        from .tool import simple_distribution
        level = _check_level(what, level)
        if probs is not None:                                   # None: a caller without probabilities
            try:
                probs = np.atleast_1d(np.asarray(probs, dtype=np.float64)).reshape(-1)
            except (TypeError, ValueError):
                raise ValueError("{}: probs must be numbers in [0, 1], got {!r}".format(what, probs))
            if probs.size == 0 or not np.all((probs >= 0.0) & (probs <= 1.0)):          # NaN fails both comparisons
                raise ValueError("{}: probs must be numbers in [0, 1], got {!r}".format(what, probs.tolist()))
        if moments_fns is None and densities is not None:
            moments_fns = [d[3]._base for d in densities]
        fns, B, k, seed = self._component_bootstrap_args(what, n_subsamples, sample_vector, moments_fns, seed)
        if densities is None:
            densities = self.construct_densities(tol, reg_param, orth_moments_tol, fns)
        if len(densities) != len(fns):
            raise ValueError("{}: {} densities for {} components".format(what, len(densities), len(fns)))
        n, s, _ = qe.bootstrap_component_moments(self._quantity, fns, B, k, seed)
        if np.any(np.sum(n, axis=1) == 0):
            raise Exception("All samples were masked")
        M, R = len(fns), int(fns[0].size)
        nf = n.astype(np.float64)
        distrs = []
        for b in range(B):
            for m in range(M):
                mobj = densities[m][3]
                with np.errstate(all="ignore"):                     # (a level whose picks were all masked: NaN, a failed solve)
                    mu = np.sum([(s[b, l, m, :R] / nf[b, l, m]) @ mobj._base_matrix.T for l in range(len(k)) if k[l] > 0], axis=0)
                distrs.append(simple_distribution.SimpleDistribution(mobj, np.stack((mu, np.ones(mobj.size)), axis=1),
                                                                     domain=mobj.domain))
        results = simple_distribution.estimate_densities_minimize(distrs, tol, reg_param)
        success = np.array([bool(r.success) for r in results], dtype=bool).reshape(B, M)
        return probs, densities, distrs, success, seed, level

    @staticmethod
    def _resampled_corr_arg(what, corr):
        if corr is not None and not (isinstance(corr, str) and corr == "scores"):
            if isinstance(corr, str):
                raise ValueError("{}: corr must be None or 'scores', got {!r}".format(what, corr))
            raise ValueError("{}: corr must be None or 'scores': a given correlation matrix has nothing to resample".format(what))

    def est_bootstrap_component_covariance(self, n_subsamples=100, sample_vector=None, seed=None, centered=True, corr=None,
                                           densities=None, tol=1e-8, reg_param=0.0, orth_moments_tol=1e-4, moments_fns=None):
        """Bootstrap replicates of the multilevel covariance and correlation between the M scalar components of the quantity, every
        replicate from one device pass per stored chunk (mlmc_bootstrap_create_xcov), seeded.  The weights are those of
        est_bootstrap_batch / est_bootstrap_components with the same seed and sample_vector: replicate b here and replicate b there
        are the same picks.  Bit-identical from run to run; the first B replicates do not depend on n_subsamples.

        corr=None: the raw components.  centered=True: the sums are shifted by a = estimate_mean(quantity).mean (as
        estimate_component_covariance; the shift only spares the sums the cancellation of raw second moments), every replicate is
        then centred on its OWN mean: cov_b = S_b - m_b m_b^T.  centered=False: no shift, and `cov` holds the raw second moments.
        corr="scores": the normal scores of the components under `densities` (constructed if missing).  The transform stays
        fixed; only the samples are resampled.  A correlation matrix is an error: there is nothing to resample.
        :return: CovarianceBootstrapReplicates(n_samples [B, L], mean [B, M], cov [B, M, M], corr [B, M, M], ok [B], seed); see
            covariance_replicates for the arithmetic.  ok[b] False (a level without a kept pick, a variance that is not positive
            and finite) leaves NaN rows; it is not an exception."""
        what = "est_bootstrap_component_covariance"
        self._resampled_corr_arg(what, corr)
        B, k, seed = self._bootstrap_args(what, n_subsamples, sample_vector, seed)
        M = int(self._quantity.size())
        shift, scores = None, None
        if corr == "scores":
            if densities is None:
                densities = self.construct_densities(tol, reg_param, orth_moments_tol, moments_fns)
            densities = list(densities)
            if len(densities) != M:
                raise ValueError("{}: {} densities for {} components".format(what, len(densities), M))
            scores = [d[0] for d in densities]
        elif centered:
            shift = np.asarray(qe.estimate_mean(self._quantity).mean, dtype=np.float64).reshape(M)
        n, s1, s2 = qe.bootstrap_component_covariance(self._quantity, B, k, seed, shift=shift, scores=scores)
        mean, cov, corr_b, ok = covariance_replicates(n, s1, s2, k, shift, centered or scores is not None)
        return CovarianceBootstrapReplicates(n, mean, cov, corr_b, ok, seed)

    def bootstrap_component_correlation(self, n_subsamples=100, sample_vector=None, seed=None, level=0.9, corr=None, densities=None,
                                        tol=1e-8, reg_param=0.0, orth_moments_tol=1e-4, moments_fns=None):
        """Bootstrap confidence bands of the correlation matrix the Gaussian copula takes (`sample_joint`): how far every entry moves
        under resampling of the stored samples.
        :param corr: None (the Pearson correlation of the components) or "scores" (estimate_score_correlation under `densities`)
        :param level: coverage of the band, 0 < level < 1
        :return: CorrelationBands(corr [M, M] the estimate's own matrix, lo, hi [M, M] = the percentiles of quantile_bands and
            std [M, M] (ddof = 1) over the ok replicates, replicates [B, M, M] = est_bootstrap_component_covariance(...).corr,
            ok [B], n_ok, seed)"""
        what = "bootstrap_component_correlation"
        level = _check_level(what, level)
        self._resampled_corr_arg(what, corr)
        B, k, seed = self._bootstrap_args(what, n_subsamples, sample_vector, seed)
        corr0, densities = self._copula_correlation(what, corr, densities, tol, reg_param, orth_moments_tol, moments_fns)
        r = self.est_bootstrap_component_covariance(B, k, seed, corr=corr, densities=densities, tol=tol, reg_param=reg_param,
                                                    orth_moments_tol=orth_moments_tol, moments_fns=moments_fns)
        lo, hi = _band_over_ok(r.corr, r.ok, level)
        n_ok = int(np.sum(r.ok))
        std = np.std(r.corr[r.ok], axis=0, ddof=1) if n_ok > 1 else np.full(r.corr.shape[1:], np.nan)
        return CorrelationBands(np.asarray(corr0, dtype=np.float64), lo, hi, std, r.corr, r.ok, n_ok, seed)

    def bootstrap_joint_probability(self, lower, upper, n_subsamples=100, sample_vector=None, seed=None, level=0.9, n=2 ** 12,
                                    seeds=tuple(range(8)), corr=None, marginals="fixed", densities=None, tol=1e-8, reg_param=0.0,
                                    orth_moments_tol=1e-4, moments_fns=None, dof=None, order="natural"):
        """Bootstrap confidence bands of estimate_joint_probability: how far the probability of a box moves when the stored samples
        are resampled.  The `stderr` of estimate_joint_probability is the quasi-Monte Carlo integration error alone; the band here
        is the sampling uncertainty of the correlation matrix (and, on request, of the marginals) pushed through the box integral.

        Replicate b is joint_probabilities(distrs_b, lower, upper, n, seeds, corr=corr_b) with corr_b replicate b of
        est_bootstrap_component_covariance(seed=seed), with the SAME quasi-Monte Carlo seeds for all, so the integration error is
        largely common to the replicates and does not widen the band.
        :param marginals: "fixed": distrs_b are the estimate's densities, only the dependence is resampled.  The estimate and all
            replicates are then the boxes of ONE device call with one factor per box
            (tool.simple_distribution.joint_probabilities_over_correlations): the limit scores are shared, replicate b brings the
            factor of corr_b.  Every number is bit for bit that of one call per replicate.  "resampled":
            distrs_b are replicate b's maximum-entropy densities, the replicate densities of bootstrap_component_quantiles with
            the same seed and sample_vector -- the same picks, so replicate b is one coherent resample of marginals and dependence.
            This keeps one call per replicate: the limit scores and the set of constrained components differ between replicates
        :param order: "natural" (default) or "genz": Genz's variable reordering of every (replicate, box) pair, as in
            estimate_joint_probability
        :param corr: None (Pearson) or "scores"; a matrix is an error (nothing to resample)
        :param n, seeds: as in estimate_joint_probability (smaller default n: there are n_subsamples + 1 integrals)
        :param dof: as in estimate_joint_probability: the Student-t copula with that many degrees of freedom.  The degrees of
            freedom are HELD FIXED over the replicates: the band is the uncertainty of the correlation (and marginals) at the given
            dof, not that of the fit of `estimate_copula_dof`.  The resampled correlation is the Pearson or scores one, which
            estimates the t copula's matrix only approximately (the quadrant correlation is not resampled).  The band keeps PLAIN
            mixing (estimate_joint_probability(mixing="plain")): under dof it shares that entry's limit on boxes that only a rare
            mixing scale reaches; for those take the point estimate from estimate_joint_probability(mixing="conditioned")
        :return: ProbabilityBands(prob [n_boxes], stderr [n_boxes] = those of estimate_joint_probability with the same n and seeds,
            lo, hi [n_boxes] = quantile_bands over the ok replicates, replicates [B, n_boxes], ok [B], n_ok, seed).  A replicate
            whose correlation is not ok, whose solve failed for a component that a box constrains (a finite limit on either
            side), or whose call raises is not ok and is left out of the bands.  `given` is not supported here."""
        from .tool import simple_distribution
        what = "bootstrap_joint_probability"
        level = _check_level(what, level)
        dof = simple_distribution._check_dof(what, dof)
        simple_distribution._check_order(what, order)
        if marginals not in ("fixed", "resampled"):
            raise ValueError("{}: marginals must be 'fixed' or 'resampled', got {!r}".format(what, marginals))
        self._resampled_corr_arg(what, corr)
        n, seeds, _ = simple_distribution._box_call_args(what, n, seeds, 0)
        seeds = [int(v) for v in seeds]
        lower = np.asarray(lower, dtype=np.float64)
        upper = np.asarray(upper, dtype=np.float64)
        if np.any(np.isnan(lower)) or np.any(np.isnan(upper)):
            raise ValueError(what + ": a limit is NaN (use -inf / +inf for a side without a limit)")
        B, k, seed = self._bootstrap_args(what, n_subsamples, sample_vector, seed)
        M = int(self._quantity.size())
        if densities is None:
            densities = self.construct_densities(tol, reg_param, orth_moments_tol, moments_fns)
        densities = list(densities)
        if len(densities) != M:
            raise ValueError("{}: {} densities for {} components".format(what, len(densities), M))
        corr0, _ = self._copula_correlation(what, corr, densities, tol, reg_param, orth_moments_tol, moments_fns)
        distrs = [d[0] for d in densities]
        if marginals == "fixed":
            # the estimate and the ok replicates: the boxes of one device call, one factor per box
            reps = self.est_bootstrap_component_covariance(B, k, seed, corr=corr, densities=densities)
            ok = reps.ok.copy()
            at = np.flatnonzero(ok)
            corrs = np.concatenate([np.asarray(corr0, dtype=np.float64)[None], reps.corr[at]], axis=0)
            results, fine = simple_distribution.joint_probabilities_over_correlations(distrs, lower, upper, n, seeds, corrs, dof=dof,
                                                                                      order=order)
            base = results[0]
            replicates = np.full((B, np.size(base.prob)), np.nan)
            ok[at[~fine[1:]]] = False
            for b, res in zip(at, results[1:]):
                if res is not None:
                    replicates[b] = res.prob
            lo, hi = _band_over_ok(replicates, ok, level)
            return ProbabilityBands(np.asarray(base.prob), np.asarray(base.stderr), lo, hi, replicates, ok, int(np.sum(ok)), seed)
        base = simple_distribution.joint_probabilities(distrs, lower, upper, n, seeds, corr=corr0, dof=dof, order=order)
        reps = self.est_bootstrap_component_covariance(B, k, seed, corr=corr, densities=densities)
        ok = reps.ok.copy()
        rep_distrs, success = None, None
        if marginals == "resampled":
            _, _, rep_distrs, success, _, _ = self._bootstrap_replicate_densities(what, None, B, k, seed, level, tol, reg_param,
                                                                                  orth_moments_tol, moments_fns, densities)
            lo_b, up_b = np.broadcast_to(lower, (np.size(base.prob), M)), np.broadcast_to(upper, (np.size(base.prob), M))
            constrained = np.any(np.isfinite(lo_b) | np.isfinite(up_b), axis=0)
            ok &= np.all(success[:, constrained], axis=1)
        replicates = np.full((B, np.size(base.prob)), np.nan)
        for b in range(B):
            if not ok[b]:
                continue
            d_b = distrs if rep_distrs is None else rep_distrs[b * M:(b + 1) * M]
            try:
                replicates[b] = simple_distribution.joint_probabilities(d_b, lower, upper, n, seeds, corr=reps.corr[b], dof=dof,
                                                                        order=order).prob
            except Exception:
                ok[b] = False
        lo, hi = _band_over_ok(replicates, ok, level)
        return ProbabilityBands(np.asarray(base.prob), np.asarray(base.stderr), lo, hi, replicates, ok, int(np.sum(ok)), seed)

    def bootstrap_joint_exceedance(self, thresholds, n_subsamples=100, sample_vector=None, seed=None, level=0.9, n=2 ** 12,
                                   seeds=tuple(range(8)), corr=None, marginals="fixed", densities=None, tol=1e-8, reg_param=0.0,
                                   orth_moments_tol=1e-4, moments_fns=None, dof=None, order="natural"):
        """P(X_m > t_m for all constrained m) with its bootstrap band: `bootstrap_joint_probability` with lower = thresholds and
        upper = +inf.
        :param thresholds: broadcast to [n_boxes, M]; -inf leaves a component unconstrained
        :param dof: the Student-t copula, its degrees of freedom held fixed over the replicates (bootstrap_joint_probability); the
            band keeps PLAIN mixing, as there
        :param order: as in bootstrap_joint_probability
        :return: as bootstrap_joint_probability"""
        t = np.asarray(thresholds, dtype=np.float64)
        if np.any(np.isnan(t)):
            raise ValueError("bootstrap_joint_exceedance: a threshold is NaN (use -inf for a component without a threshold)")
        return self.bootstrap_joint_probability(t, np.inf, n_subsamples=n_subsamples, sample_vector=sample_vector, seed=seed,
                                                level=level, n=n, seeds=seeds, corr=corr, marginals=marginals, densities=densities,
                                                tol=tol, reg_param=reg_param, orth_moments_tol=orth_moments_tol, moments_fns=moments_fns,
                                                dof=dof, order=order)

    def bs_target_var_n_estimated(self, target_var, sample_vec=None, *, batch=False, seed=None):
        """batch=True: the 300 replicates come from est_bootstrap_batch(300, sample_vec, seed=seed)."""
        sample_vec = determine_sample_vec(n_collected_samples=self._sample_storage.get_n_collected(),
                                          n_levels=self._sample_storage.get_n_levels(), sample_vector=sample_vec)
        if batch:
            self.est_bootstrap_batch(n_subsamples=300, sample_vector=sample_vec, seed=seed)
        else:
            self.est_bootstrap(n_subsamples=300, sample_vector=sample_vec)
        variances, n_ops = self.estimate_diff_vars_regression(sample_vec, raw_vars=self.mean_bs_l_vars)
        return estimate_n_samples_for_target_variance(target_var, variances, n_ops,
                                                      n_levels=self._sample_storage.get_n_levels())

    # ---- domain ------------------------------------------------------------------------------------------
    @staticmethod
    def estimate_domain(quantity, sample_storage, quantile=None):
        """Moments domain from sample quantiles of the fine samples (reference: :275-302).  As in the reference,
        `chunks(n_samples=...)` without a level id yields the level-0 chunk for every level."""
        if quantile is None:
            quantile = 0.01
        ranges = []
        for level_id in range(sample_storage.get_n_levels()):
            chunk_spec = next(sample_storage.chunks(n_samples=sample_storage.get_n_collected()[level_id]))
            fine = qe.fine_samples_for_device(quantity, chunk_spec)
            # NaN removal + np.percentile of the reference (:298-299) as one device call (exact radix select)
            ranges.append(engine.percentiles(fine, [100 * quantile, 100 * (1 - quantile)]))
        ranges = np.array(ranges)
        return np.min(ranges[:, 0]), np.max(ranges[:, 1])

    @staticmethod
    def estimate_domains(quantity, sample_storage, quantile=None):
        """-> [M, 2]: row m is estimate_domain(scalar_component(quantity, m), sample_storage, quantile), bit for bit (row order
        as construct_densities documents; a scalar quantity gives [[lo, hi]]).  The quantity is evaluated once per level for
        all components and the percentiles of all of them come from one device call (engine.row_percentiles); NaNs are
        removed per component.  Same chunks as estimate_domain."""
        if quantile is None:
            quantile = 0.01
        n_comp = int(quantity.size())
        ranges = []
        for level_id in range(sample_storage.get_n_levels()):
            chunk_spec = next(sample_storage.chunks(n_samples=sample_storage.get_n_collected()[level_id]))
            fine = qe.fine_samples_for_device(quantity, chunk_spec)
            ranges.append(engine.row_percentiles(fine.reshape(n_comp, -1), [100 * quantile, 100 * (1 - quantile)]))
        return _domains_of(ranges)

    # ---- PDF ---------------------------------------------------------------------------------------------
    def construct_density(self, tol=1e-8, reg_param=0.0, orth_moments_tol=1e-4, exact_pdf=None):
        """Maximum-entropy density from the estimated moments (reference: :304-331).
        -> (distr_obj, info, result, moments_obj)"""
        from .tool import simple_distribution
        if not isinstance(self._quantity.qtype, ScalarType):
            raise NotImplementedError("Currently, we only support ScalarType quantities")
        # only the means of the two estimates are used (the reference overwrites the variances with ones, :323)
        cov_mat = qe.estimate_mean(qe.covariance(self._quantity, self._moments_fn), variance=False).mean
        moments_obj, info = simple_distribution.construct_ortogonal_moments(self._moments_fn, cov_mat, tol=orth_moments_tol)
        est_moments = qe.estimate_mean(qe.moments(self._quantity, moments_obj), variance=False).mean
        est_vars = np.ones(moments_obj.size)        # the reference discards the estimated variances (:323)
        moments_data = np.stack((est_moments, est_vars), axis=1)
        distr_obj = simple_distribution.SimpleDistribution(moments_obj, moments_data, domain=moments_obj.domain)
        result = distr_obj.estimate_density_minimize(tol, reg_param)
        return distr_obj, info, result, moments_obj

    def construct_densities(self, tol=1e-8, reg_param=0.0, orth_moments_tol=1e-4, moments_fns=None):
        """Maximum-entropy density of EVERY scalar component of the quantity (any qtype, scalar included).

        Entry m of the returned list is what `Estimate(q_m, storage, fn_m).construct_density(tol, reg_param,
        orth_moments_tol)` returns for the scalar sub-quantity q_m = row m of `quantity.samples(chunk)` ([M, n, 2]): each
        component is NaN-masked and domain-clipped on its own (a NaN in component 3 does not drop that sample from
        component 0 -- unlike `mask_nan_samples` over the whole vector).  Row order: the qtype flattened from the outside in,
        e.g. for the result format dict -> time series -> field -> array, m = ((time_index * n_locations + location_index)
        * array_size + flat_array_index) inside the dict entry's block, dict entries one after another in their order.
        For Legendre / monomial / Fourier moments (one family and size for all components) both estimates of every
        component come from ONE device pass per stored chunk (mlmc_accum_estimate_multi); other moments (splines, transformed
        moments, MLMC_HIP_LINEARIZE=0) take the scalar chain per component, with the same results.  The orthogonalisation
        stays per component on the host; the max-entropy problems of all components are solved in ONE batched device call
        (tool.simple_distribution.estimate_densities_minimize).  That solve gives one workgroup to each problem: it beats
        M cooperative single solves from M ~ 16 components on, below that construct_density per component is faster.
        :param moments_fns: optional list of M moments objects (component m uses moments_fns[m]); default: this
            Estimate's moments_fn for every component
        :return: list of M tuples (distr_obj, info, result, moments_obj)"""
        from .tool import simple_distribution
        n_comp = int(self._quantity.size())
        if moments_fns is None:
            moments_fns = [self._moments_fn] * n_comp
        moments_fns = list(moments_fns)
        if len(moments_fns) != n_comp:
            raise ValueError("construct_densities: {} moments objects for {} components".format(len(moments_fns), n_comp))
        exts = qe.linearized_bases(moments_fns)
        if exts is not None:
            # ONE device pass per stored chunk for all components: level sums of the extended moments of every component
            # (its own mask) give both means -- the covariance by the product linearisation, the orthogonal moments as
            # T_m times the first R sums -- as the scalar chain takes them from its first estimate (quantity_estimate.py)
            n, _, sums = qe.multi_component_sums(self._quantity, exts)
            if np.any(np.sum(n, axis=0) == 0):
                raise Exception("All samples were masked")
            nf = n.astype(np.float64)

            def level_mean(m, s):                          # sum over levels of s_l / n_l (engine.level_stats)
                return np.sum(s / nf[:, m, None], axis=0)
            cov_means = [level_mean(m, linearize.covariance_sums_from_moment_sums(fn, sums[:, m, :])).reshape(fn.size, fn.size)
                         for m, fn in enumerate(moments_fns)]
        else:
            comps = [self._quantity] if isinstance(self._quantity.qtype, ScalarType) else \
                [scalar_component(self._quantity, m) for m in range(n_comp)]
            cov_means = qe.component_means(comps, moments_fns, cov=True)
        ortho = [simple_distribution.construct_ortogonal_moments(fn, cov, tol=orth_moments_tol)
                 for fn, cov in zip(moments_fns, cov_means)]
        if exts is not None:
            mom_means = [level_mean(m, sums[:, m, :fn.size] @ mobj._base_matrix.T)
                         for m, (fn, (mobj, _)) in enumerate(zip(moments_fns, ortho))]
        else:
            mom_means = qe.component_means(comps, [m for m, _ in ortho], cov=False)
        distrs = []
        for (moments_obj, _), est_moments in zip(ortho, mom_means):
            moments_data = np.stack((est_moments, np.ones(moments_obj.size)), axis=1)   # variances discarded (:323)
            distrs.append(simple_distribution.SimpleDistribution(moments_obj, moments_data, domain=moments_obj.domain))
        results = simple_distribution.estimate_densities_minimize(distrs, tol, reg_param)
        return [(d, info, r, m) for d, (m, info), r in zip(distrs, ortho, results)]

    def estimate_component_quantiles(self, probs, tol=1e-8, reg_param=0.0, orth_moments_tol=1e-4, moments_fns=None, densities=None):
        """Quantiles of the maximum-entropy density of EVERY scalar component of the quantity, in one batched device call
        (tool.simple_distribution.quantiles: median, 5 % / 95 % bands, credible intervals of a field).

        :param probs: probabilities, the same for every component
        :param densities: the list `construct_densities` returned; without it the method calls
            `construct_densities(tol, reg_param, orth_moments_tol, moments_fns)` itself
        :return: (q, success): q [M, len(probs)], row m = the quantiles of component m (the row order of construct_densities),
            equal to `construct_density` of `scalar_component(quantity, m)` followed by `.quantile(probs)` up to what
            construct_densities promises against the scalar chain; success [M] bool, the solver's verdict per component (rows of
            failed solves are still returned)"""
        from .tool import simple_distribution
        if densities is None:
            densities = self.construct_densities(tol, reg_param, orth_moments_tol, moments_fns)
        probs = np.atleast_1d(np.asarray(probs, dtype=np.float64)).reshape(-1)
        q = simple_distribution.quantiles([d[0] for d in densities], probs)
        success = np.array([bool(d[2].success) for d in densities], dtype=bool)
        return np.array(q, dtype=np.float64).reshape(len(densities), probs.size), success

    def sample_components(self, n, seed, tol=1e-8, reg_param=0.0, orth_moments_tol=1e-4, moments_fns=None, densities=None, first=0,
                          antithetic=False, device=False, qmc=False):
        """Seeded draws from the maximum-entropy density of EVERY scalar component of the quantity, in one batched device call
        (tool.simple_distribution.samples): draws first .. first + n - 1 of component m come from stream m under `seed`.

        The marginals are drawn INDEPENDENTLY; `sample_joint` draws them jointly, through a Gaussian copula with the
        correlation of `estimate_component_covariance`.
        :param n: draws per component
        :param seed: required, 0 <= seed < 2^64; there is no global generator
        :param densities: as in estimate_component_quantiles
        :param qmc: scrambled Sobol' points instead of pseudo-random ones (see tool.simple_distribution.samples): the streams are
            dimensions (at most 1024 components: component m is dimension m), n should be a power of two with `first` a multiple of it, and R seeds give R
            independent estimates whose spread is the error bar.  Not together with antithetic
        :param device: return the draws as a float64 torch device tensor
        :return: (samples, success): samples [M, n], row m = `.rvs(n, seed, stream=m, first=first, antithetic=antithetic)` of
            component m's distribution (the row order of construct_densities); success [M] bool, the solver's verdict per
            component (rows of failed solves are still returned)"""
        from .tool import simple_distribution
        if isinstance(n, bool) or int(n) != n or n < 0:
            raise ValueError("sample_components: n must be a non-negative integer")
        simple_distribution._sample_flags("sample_components", antithetic, qmc)
        if densities is None:
            densities = self.construct_densities(tol, reg_param, orth_moments_tol, moments_fns)
        flat, _, _ = simple_distribution._samples_flat([d[0] for d in densities], int(n), seed, None, first, antithetic, device, False, qmc)
        success = np.array([bool(d[2].success) for d in densities], dtype=bool)
        return flat.reshape(len(densities), int(n)), success           # the call's one array, viewed as [M, n]

    def estimate_score_correlation(self, tol=1e-8, reg_param=0.0, orth_moments_tol=1e-4, moments_fns=None, densities=None):
        """Multilevel correlation of the NORMAL SCORES z_m = Phi^-1(Fhat_m(X_m)) of the components under their maximum-entropy
        marginals: the correlation a Gaussian copula over these marginals takes (`sample_joint(corr="scores")`).  One pass over
        the stored samples: every fine and coarse value goes through its component's CDF and Phi^-1 on the device
        (mlmc_density_scores_batch) right before the component-covariance kernel; the scores never leave the device
        (quantity_estimate.component_covariance(scores=...)).  A sample with a NaN or a value outside the open domain of its
        marginal in any component, fine or coarse, is dropped from the whole matrix (n_rm_samples counts them).
        :param densities: as in estimate_component_quantiles
        :return: ScoreCorrelation(corr, cov, cov_var, mean, var, n_samples, n_rm_samples):
            corr [M, M]: cov_ij / sqrt(cov_ii cov_jj), unit diagonal;
            cov [M, M], cov_var [M, M]: the multilevel second moments of the scores minus mean mean^T, and the variance of the
                estimate of the second moments (sum over levels of l_vars / n_l);
            mean [M], var [M]: multilevel mean and variance of each component's scores.  They are 0 and 1 when a density fits its
                in-domain samples, so they are a free calibration check of every marginal: a mean far from 0 or a variance far
                from 1 (against sqrt(cov_var)) says that the density of that component does not describe its samples;
            n_samples [L], n_rm_samples [L]: kept and dropped samples per level.
        A component whose var is not positive and finite is an error that names it."""
        if isinstance(densities, str):
            raise ValueError("estimate_score_correlation: densities must be the list construct_densities returned")
        if densities is None:
            densities = self.construct_densities(tol, reg_param, orth_moments_tol, moments_fns)
        M = int(self._quantity.size())
        densities = list(densities)
        if len(densities) != M:
            raise ValueError("estimate_score_correlation: {} densities for {} components".format(len(densities), M))
        distrs = [d[0] for d in densities]
        r = qe.estimate_mean(qe.component_covariance(self._quantity, scores=distrs))
        second = np.asarray(r.mean, dtype=np.float64).reshape(M + 1, M + 1)
        mean = second[M, :M].copy()
        cov = second[:M, :M] - mean[:, None] * mean[None, :]
        cov = 0.5 * (cov + cov.T)
        cov_var = np.asarray(r.var, dtype=np.float64).reshape(M + 1, M + 1)[:M, :M].copy()
        var = np.diag(cov).copy()
        bad = np.flatnonzero(~(np.isfinite(var) & (var > 0)))
        if bad.size:
            raise ValueError("estimate_score_correlation: component {} has no positive finite variance estimate of its scores "
                             "({})".format(int(bad[0]), var[bad[0]]))
        sd = np.sqrt(var)
        corr = cov / sd[:, None] / sd[None, :]
        np.fill_diagonal(corr, 1.0)
        return ScoreCorrelation(corr, cov, cov_var, mean, var, np.asarray(r.n_samples, dtype=np.int64),
                                np.asarray(r.n_rm_samples, dtype=np.int64))

    def _copula_correlation(self, what, corr, densities, tol, reg_param, orth_moments_tol, moments_fns):
        """the correlation matrix of the normal scores that `corr` of sample_joint / sample_conditional stands for: None = the
        Pearson correlation of the components, "scores" = estimate_score_correlation with the densities (constructed here if
        need be), "quadrant" = estimate_quadrant_correlation with the densities, a matrix = itself.
        "quadrant" counts how often two components lie above their medians at once, and has about four times the standard error
        of the Pearson and scores routes (0.0053 - 0.0061 against 0.0013 - 0.0016 at 2 x 2^18 samples of three components).  It is
        the one that stays consistent under a Student-t copula: the quadrant probability is 1/4 + asin(rho) / (2 pi) for every
        elliptical copula, while the correlation of the normal scores of t-copula samples is not the copula's rho.  Like every
        matrix it goes through tool.simple_distribution.correlation_factor, which repairs an indefinite estimate.
        :return: (corr, densities), densities as passed in unless "scores" / "quadrant" had to construct them"""
        if isinstance(corr, str):
            if corr not in ("scores", "quadrant"):
                raise ValueError("{}: corr must be None, 'scores' or a correlation matrix, or 'quadrant', got {!r}".format(what, corr))
            if densities is None:
                densities = self.construct_densities(tol, reg_param, orth_moments_tol, moments_fns)
            if corr == "scores":
                corr = self.estimate_score_correlation(densities=densities).corr
            else:
                corr = self.estimate_quadrant_correlation(densities=densities).corr
        elif corr is None:
            cov, _ = self.estimate_component_covariance()
            var = np.diag(cov)
            bad = np.flatnonzero(~(np.isfinite(var) & (var > 0)))
            if bad.size:
                raise ValueError("{}: component {} has no positive finite variance estimate ({})".format(what, int(bad[0]),
                                                                                                         var[bad[0]]))
            sd = np.sqrt(var)
            corr = cov / sd[:, None] / sd[None, :]
            np.fill_diagonal(corr, 1.0)
        return corr, densities

    def sample_joint(self, n, seed, corr=None, tol=1e-8, reg_param=0.0, orth_moments_tol=1e-4, moments_fns=None, densities=None, first=0,
                     antithetic=False, device=False, qmc=False, dof=None):
        """Seeded JOINT draws of all scalar components of the quantity, in one batched device call
        (tool.simple_distribution.joint_samples): the maximum-entropy marginals of `construct_densities` joined by a Gaussian
        copula.  Column j of the result is one scenario of the whole vector: use it for the sum of the components, the CVaR of a
        portfolio of outputs or joint exceedance (small joint probabilities: `estimate_joint_exceedance`, which does not count).

        What the dependence is: the copula takes the correlation of the NORMAL SCORES Phi^-1(F_m(X_m)), and there are two
        estimates of it to choose from.
        corr=None: the PEARSON correlation of the components (corr_ij = cov_ij / sqrt(cov_ii cov_jj) of
        `estimate_component_covariance()`) is used in its place.  This is the uncorrected Nataf / NORTA approximation: it is
        exact for Gaussian marginals and costs no density, but for other marginals the draws are less dependent than the data.
        corr="scores": the multilevel correlation of the normal scores themselves (`estimate_score_correlation` with the same
        densities): one more pass over the stored samples through Phi^-1(Fhat_m(.)) on the device.  The two agree for
        near-Gaussian marginals and differ where the marginals are skewed or heavy on one side: for two truncated exponentials of
        opposite skew joined at a score correlation of 0.8 the Pearson correlation is about 0.54, which corr=None would feed back into
        the copula.  Prefer "scores" unless the marginals are close to Gaussian.
        A correlation estimate that is not positive definite (a telescoping sum need not be) is repaired by
        `tool.simple_distribution.correlation_factor`.
        :param n: draws per component, indices first .. first + n - 1
        :param seed: required, 0 <= seed < 2^64; there is no global generator.  With corr = identity the draws equal those of
            `sample_components` with the same seed up to rounding: use another seed where the two must be independent
        :param corr: None, "scores", or a correlation matrix [M, M] of the normal scores
        :param densities: as in estimate_component_quantiles
        :param qmc: scrambled Sobol' points instead of pseudo-random ones (see tool.simple_distribution.joint_samples): the streams are
            dimensions (at most 1024 latent normals: latent normal k is dimension k), n should be a power of two with `first` a multiple of it, and R seeds give R
            independent estimates whose spread is the error bar.  Not together with antithetic
        :param device: return the draws as a float64 torch device tensor
        :param dof: None or np.inf: the Gaussian copula; a float in [1, 64]: a Student-t copula with that many degrees of freedom
            (`estimate_copula_dof` fits it), whose mixing variable takes stream M.  `corr` is then the t copula's correlation
            matrix, which corr="quadrant" estimates consistently; None and "scores" estimate it only approximately
        :return: (samples [M, n], success [M], corr_used [M, M]): row m = component m (the row order of construct_densities);
            the solver's verdict per component; F F^T of the factor that was used"""
        from .tool import simple_distribution
        if isinstance(n, bool) or int(n) != n or n < 0:
            raise ValueError("sample_joint: n must be a non-negative integer")
        simple_distribution._sample_flags("sample_joint", antithetic, qmc)
        simple_distribution._check_dof("sample_joint", dof)
        corr, densities = self._copula_correlation("sample_joint", corr, densities, tol, reg_param, orth_moments_tol, moments_fns)
        factor, _ = simple_distribution.correlation_factor(corr)
        if densities is None:
            densities = self.construct_densities(tol, reg_param, orth_moments_tol, moments_fns)
        draws = simple_distribution.joint_samples([d[0] for d in densities], int(n), seed, factor=factor, first=first,
                                                  antithetic=antithetic, device=device, qmc=qmc, dof=dof)
        success = np.array([bool(d[2].success) for d in densities], dtype=bool)
        return draws, success, factor @ factor.T

    def sample_conditional(self, n, seed, given, corr=None, tol=1e-8, reg_param=0.0, orth_moments_tol=1e-4, moments_fns=None,
                           densities=None, first=0, antithetic=False, device=False, qmc=False, dof=None):
        """Seeded joint draws of the components that are not in `given`, CONDITIONAL on measured or fixed values of the others, in
        one batched device call (tool.simple_distribution.conditional_samples): the marginals and the Gaussian copula of
        `sample_joint`, with the scores of the given components fixed at Phi^-1(Fhat_o(x_o)).  Scenarios of the rest of a field
        given the head at an observation well, of the rest of a series given its first steps.
        :param given: mapping component index -> value, or -> array [B] for B sets of values at once (a what-if fan); the tables
            of the marginals and the latent normals are made once for all sets
        :param corr: as in sample_joint: None (Pearson), "scores", or a correlation matrix [M, M] of the normal scores
        :param densities: as in estimate_component_quantiles
        :param qmc: scrambled Sobol' points instead of pseudo-random ones (see tool.simple_distribution.conditional_samples): the streams are
            dimensions (at most 1024 latent normals: latent normal k is dimension k), n should be a power of two with `first` a multiple of it, and R seeds give R
            independent estimates whose spread is the error bar.  Not together with antithetic
        :param dof: None or np.inf: the Gaussian copula; a float in [1, 64]: the Student-t copula of `sample_joint(dof=...)`
            (tool.simple_distribution.conditional_samples(dof=...)), under which an extreme given value widens the law of the other
            components.  `corr` is then the t copula's correlation matrix, as in sample_joint ("quadrant" estimates it
            consistently); dof + the number of given components must not exceed 192; the mixing variable takes the stream after
            those of the latent normals
        :return: (samples, success [M], ConditionalFactorInfo): samples [M, n] for scalar values and [B, M, n] for arrays, rows
            of given components hold the given values; the solver's verdict per component; the components that were drawn,
            their conditional standard deviations in score space and what `correlation_factor` did to the matrix"""
        from .tool import simple_distribution
        if isinstance(n, bool) or int(n) != n or n < 0:
            raise ValueError("sample_conditional: n must be a non-negative integer")
        simple_distribution._sample_flags("sample_conditional", antithetic, qmc)
        nu = simple_distribution._check_dof("sample_conditional", dof)
        simple_distribution._check_conditional_dof("sample_conditional", nu, len(given) if hasattr(given, "items") else 0)
        corr, densities = self._copula_correlation("sample_conditional", corr, densities, tol, reg_param, orth_moments_tol, moments_fns)
        if densities is None:
            densities = self.construct_densities(tol, reg_param, orth_moments_tol, moments_fns)
        distrs = [d[0] for d in densities]
        observed = simple_distribution._parse_given("sample_conditional", given, len(distrs))[0]
        cond = simple_distribution.conditional_factor(corr, observed, return_observed=nu is not None)
        draws = simple_distribution.conditional_samples(distrs, int(n), seed, given, factor_info=cond, first=first,
                                                        antithetic=antithetic, device=device, qmc=qmc, dof=dof)
        success = np.array([bool(d[2].success) for d in densities], dtype=bool)
        return draws, success, cond[2]

    def estimate_joint_probability(self, lower, upper, n=2 ** 14, seeds=tuple(range(8)), corr=None, given=None, tol=1e-8, reg_param=0.0,
                                   orth_moments_tol=1e-4, moments_fns=None, densities=None, first=0, qmc=True, dof=None, mixing="plain",
                                   order="natural"):
        """Probability that the components lie in a box AT ONCE, P(lower_m < X_m < upper_m for all m), under the marginals and the
        Gaussian copula of `sample_joint`, for B boxes in one batched device call (tool.simple_distribution.joint_probabilities):
        Genz's separation of variables on scrambled Sobol' points.  Its error is relative and falls like 1 / n, so the small
        probabilities of a reliability question (1e-4 .. 1e-8) are resolved, where counting the scenarios of `sample_joint`
        would need 1e8 .. 1e12 draws.  Components that no box constrains (limits -inf / +inf) are dropped before the
        factorisation and cost nothing.
        :param lower, upper: broadcast to [B, M] in the components' own units; with `given` to [B, q] over the components that are
            not given.  +-inf, or a value at or beyond an end of the component's domain, does not constrain that side
        :param n: points per seed; a power of two with `first` a multiple of it
        :param seeds: one independent scramble each; the spread of their means is the error bar
        :param corr: as in sample_joint: None (Pearson), "scores", or a correlation matrix [M, M] of the normal scores
        :param given: None, or as in sample_conditional: the probability is conditional on the given values; arrays [B] pair
            with the boxes
        :param densities: as in estimate_component_quantiles
        :param qmc: False: Philox uniforms instead of Sobol' points (plain Monte Carlo over the unit cube)
        :param dof: None or np.inf: the Gaussian copula, bit for bit.  A float in [1, 64]: the STUDENT-T copula of
            `sample_joint(dof=...)` with that many degrees of freedom (`estimate_copula_dof` fits it), by Genz and Bretz's mixing
            variable: one more coordinate per point, the same relative accuracy in the tail.  Where `estimate_tail_dependence`
            shows joint tails (a large positive z), this is the number to use: the Gaussian one is too small.  `corr` is then the t
            copula's correlation matrix, which corr="quadrant" estimates consistently; None and "scores" only approximately.  Not
            together with `given`: that is `estimate_conditional_probability`
        :param mixing: "plain" (default, bit for bit as before) or "conditioned" (dof only, not with `given`): the component with the
            smallest marginal probability of each box LEADS: it is drawn inside its limits and the mixing scale follows its law given
            that draw (tool.simple_distribution.joint_probabilities / event_samples), so the relative error holds at any depth of
            the box.  Plain mixing returns a number that is orders of magnitude too small, with a `stderr` that does not show it,
            once only a rare mixing scale reaches the box (marginal levels of 1e-6 at dof = 3)
        :param order: "natural" (default, bit for bit as before): the chain integrates the constrained components in their own
            order.  "genz": Genz's variable reordering of every box on the device (tool.simple_distribution.box_order), still one
            chain call: the same probability with a `stderr` that is orders of magnitude smaller where the limits differ much
            between correlated components.  Independent components gain nothing
        :return: (JointProbability(prob [B], stderr [B], replicates [R, B], n, seeds), success [M])"""
        from .tool import simple_distribution
        what = "estimate_joint_probability"
        dof = simple_distribution._box_dof(what, dof, None, given)
        simple_distribution._check_mixing(what, mixing, dof, None, given)
        simple_distribution._check_order(what, order)
        return self._joint_probability(what, simple_distribution.joint_probabilities, lower, upper, n, seeds, corr, given, tol, reg_param,
                                       orth_moments_tol, moments_fns, densities, first, qmc, dof, mixing, order)

    def estimate_conditional_probability(self, lower, upper, given, n=2 ** 14, seeds=tuple(range(8)), corr=None, tol=1e-8, reg_param=0.0,
                                         orth_moments_tol=1e-4, moments_fns=None, densities=None, first=0, qmc=True, dof=None):
        """Probability that the components that are NOT in `given` lie in a box at once, CONDITIONAL on measured or fixed values of
        the others (tool.simple_distribution.conditional_probabilities): "how likely is it that the other components exceed their
        limits at once, given this value at the well?".  With dof None this is `estimate_joint_probability(given=...)`, bit for
        bit, through the same body.  With dof, a float in [1, 64], the copula is the Student-t copula of `sample_joint(dof=...)`,
        under which an extreme given value WIDENS the law of the others (the Gaussian copula cannot): given p values the t scores
        of the others are multivariate t with dof + p degrees of freedom (at most 192), as in `sample_conditional(dof=...)`.
        :param lower, upper: broadcast to [B, q] over the components that are not given, ascending, in their own units
        :param given: as in sample_conditional (required); arrays [B] pair with the boxes
        :param corr: as in sample_joint; with dof corr="quadrant" is the consistent correlation, as for sample_conditional(dof=...)
        :param n, seeds, densities, first, qmc: as in estimate_joint_probability
        The conditional family keeps PLAIN mixing (there is no `mixing` keyword here): its mixing variable has dof + p degrees of
        freedom, and a conditioned lead would need the t functions at dof + p + 1, outside their tested range.
        :return: (JointProbability, success [M])"""
        from .tool import simple_distribution
        what = "estimate_conditional_probability"
        if given is None:
            raise ValueError(what + ": given is required (without given values: estimate_joint_probability)")
        nu = simple_distribution._check_dof(what, dof)
        simple_distribution._check_conditional_dof(what, nu, len(given) if hasattr(given, "items") else 0)
        return self._joint_probability(what, simple_distribution.conditional_probabilities, lower, upper, n, seeds, corr, given, tol, reg_param, orth_moments_tol, moments_fns,
                                       densities, first, qmc, nu)

    def _joint_probability(self, what, entry, lower, upper, n, seeds, corr, given, tol, reg_param, orth_moments_tol, moments_fns,
                           densities, first, qmc, dof, mixing="plain", order="natural"):
        """the one body of estimate_joint_probability and estimate_conditional_probability; dof and mixing checked by the caller
        (mixing goes to the entry only where it is not "plain": the conditional entry has no such keyword)"""
        from .tool import simple_distribution
        n, seeds, first = simple_distribution._box_call_args(what, n, seeds, first)
        if np.any(np.isnan(np.asarray(lower, dtype=np.float64))) or np.any(np.isnan(np.asarray(upper, dtype=np.float64))):
            raise ValueError(what + ": a limit is NaN (use -inf / +inf for a side without a limit)")
        corr, densities = self._copula_correlation(what, corr, densities, tol, reg_param, orth_moments_tol, moments_fns)
        if densities is None:
            densities = self.construct_densities(tol, reg_param, orth_moments_tol, moments_fns)
        more = {} if mixing == "plain" else {"mixing": mixing}
        if order != "natural":
            more["order"] = order
        result = entry([d[0] for d in densities], lower, upper, n=n, seeds=[int(s) for s in seeds], corr=corr, given=given, first=first,
                       qmc=qmc, dof=dof, **more)
        success = np.array([bool(d[2].success) for d in densities], dtype=bool)
        return result, success

    def estimate_conditional_exceedance(self, thresholds, given, n=2 ** 14, seeds=tuple(range(8)), corr=None, tol=1e-8, reg_param=0.0,
                                        orth_moments_tol=1e-4, moments_fns=None, densities=None, first=0, qmc=True, dof=None):
        """P(X_m > t_m for all constrained m that are not given | the given values): `estimate_conditional_probability` with
        lower = thresholds and upper = +inf.
        :param thresholds: broadcast to [B, q] over the components that are not given; -inf leaves a component unconstrained
        :return: as estimate_conditional_probability"""
        t = np.asarray(thresholds, dtype=np.float64)
        if np.any(np.isnan(t)):
            raise ValueError("estimate_conditional_exceedance: a threshold is NaN (use -inf for a component without a threshold)")
        return self.estimate_conditional_probability(t, np.inf, given, n=n, seeds=seeds, corr=corr, tol=tol, reg_param=reg_param,
                                                     orth_moments_tol=orth_moments_tol, moments_fns=moments_fns, densities=densities,
                                                     first=first, qmc=qmc, dof=dof)

    def estimate_joint_exceedance(self, thresholds, n=2 ** 14, seeds=tuple(range(8)), corr=None, given=None, tol=1e-8, reg_param=0.0,
                                  orth_moments_tol=1e-4, moments_fns=None, densities=None, first=0, qmc=True, dof=None, mixing="plain",
                                  order="natural"):
        """P(X_m > t_m for all constrained m): `estimate_joint_probability` with lower = thresholds and upper = +inf.
        :param thresholds: broadcast to [B, M]; -inf leaves a component unconstrained
        :param dof: the Student-t copula, as in estimate_joint_probability
        :param mixing: as in estimate_joint_probability; with dof and thresholds in the far tail use mixing="conditioned"
        :param order: as in estimate_joint_probability; "genz" pays where the thresholds differ much between correlated components
        :return: as estimate_joint_probability"""
        t = np.asarray(thresholds, dtype=np.float64)
        if np.any(np.isnan(t)):
            raise ValueError("estimate_joint_exceedance: a threshold is NaN (use -inf for a component without a threshold)")
        return self.estimate_joint_probability(t, np.inf, n=n, seeds=seeds, corr=corr, given=given, tol=tol, reg_param=reg_param,
                                               orth_moments_tol=orth_moments_tol, moments_fns=moments_fns, densities=densities,
                                               first=first, qmc=qmc, dof=dof, mixing=mixing, order=order)

    def estimate_tail_dependence(self, probs=(0.9, 0.95, 0.99), tail="upper", corr=None, densities=None, tol=1e-8, reg_param=0.0,
                                 orth_moments_tol=1e-4, moments_fns=None, dof=None):
        """A check of the Gaussian copula that `sample_joint`, `estimate_joint_probability` and their relatives assume: the
        multilevel frequency with which TWO components lie beyond their p-quantile at once, for every pair, held against the
        bivariate normal orthant at the copula's own correlation.  A Gaussian copula has no tail dependence; where the stored
        samples have it, chi = P(both beyond) / (1 - p) stays above chi_model as p grows, z is large and positive, and every joint
        tail probability computed under the copula is too small.

        One pass over the stored samples: each fine and coarse value goes through its marginal's CDF on the device, a wave's
        ballot turns 64 uniforms into one word and a pair count is a popcount (quantity_estimate.component_concordance(scores=...)).
        The level difference of an indicator product is -1, 0 or 1, so the multilevel mean and its variance follow exactly from
        three integers per pair, level and probability.
        :param probs: probability levels p in (0, 1); at most 16 events per call ("both" makes two per level)
        :param tail: "upper": the events u > p; "lower": u < 1 - p (the same model value, by symmetry); "both": the upper events
            followed by the lower ones, 2 G events in one pass
        :param corr: as in sample_joint: None (Pearson), "scores", or a correlation matrix [M, M] of the normal scores
        :param densities: as in estimate_component_quantiles
        :param dof: None or np.inf: the model is the Gaussian copula's.  A float in [1, 64]: the model is the orthant of the
            Student-t copula with that many degrees of freedom (tool.simple_distribution.bivariate_t_orthant at the t score of
            p_g), the copula of `sample_joint(dof=...)`; `estimate_copula_dof` chooses it from the same counts
        :return: TailDependence(prob, var, chi, model, chi_model, z [G, M, M], marginal [G, M], counts, n_samples, n_rm_samples [L],
            corr [M, M]):
            prob, var: the multilevel estimate of P(U_a and U_b both beyond level p_g) and its variance; the diagonal of prob
                (= marginal) is P(U_a beyond p_g) and equals 1 - p when the marginal fits: a calibration of each marginal there;
            chi = prob / (1 - p); model = tool.simple_distribution.bivariate_orthant at the score of p_g and corr_ab,
                chi_model = model / (1 - p);
            z = (prob - model) / sqrt(var), NaN where var is not positive and finite, and on the diagonal;
            counts: the integers per level (quantity_estimate.ComponentConcordance).
        What z does NOT contain: the sampling error of the correlation estimate that `model` is evaluated at, and that of the
        fitted marginals that turn values into uniforms -- var is the sampling variance of the frequency alone.  So |z| of 2 or 3
        says little; a consistent sign over pairs and a growth with p says much."""
        walk = self._tail_concordance("estimate_tail_dependence", probs, tail, corr, densities, tol, reg_param, orth_moments_tol,
                                      moments_fns, dof)
        return self._tail_dependence(walk, walk["dof"])

    def _tail_concordance(self, what, probs, tail, corr, densities, tol, reg_param, orth_moments_tol, moments_fns, dof=None):
        """the arguments and the one pass of estimate_tail_dependence / estimate_copula_dof: dict(prob, var [G, M, M], levels [G],
        counts, corr [M, M], dof)"""
        from .tool import simple_distribution
        dof = simple_distribution._check_dof(what, dof)
        if tail not in ("upper", "lower", "both"):
            raise ValueError("{}: tail must be 'upper', 'lower' or 'both', got {!r}".format(what, tail))
        p = np.atleast_1d(np.asarray(probs, dtype=np.float64))
        if p.ndim != 1 or p.size == 0 or not np.all((p > 0.0) & (p < 1.0)):
            raise ValueError(what + ": probs must be probability levels in (0, 1)")
        if p.size * (2 if tail == "both" else 1) > simple_distribution._lib.CONCORDANCE_MAX_G:
            raise ValueError("{}: at most {} events per call".format(what, simple_distribution._lib.CONCORDANCE_MAX_G))
        if isinstance(densities, str):
            raise ValueError(what + ": densities must be the list construct_densities returned")
        corr, densities = self._copula_correlation(what, corr, densities, tol, reg_param, orth_moments_tol, moments_fns)
        if densities is None:
            densities = self.construct_densities(tol, reg_param, orth_moments_tol, moments_fns)
        densities = list(densities)
        M = int(self._quantity.size())
        if len(densities) != M:
            raise ValueError("{}: {} densities for {} components".format(what, len(densities), M))
        corr = np.asarray(corr, dtype=np.float64)
        if corr.shape != (M, M):
            raise ValueError("{}: corr of shape {}, expected ({}, {})".format(what, corr.shape, M, M))
        ones = np.ones((p.size, M))
        lower, upper, levels = [], [], []
        if tail in ("upper", "both"):
            lower.append(p[:, None] * ones), upper.append(np.inf * ones), levels.append(p)
        if tail in ("lower", "both"):
            lower.append(-np.inf * ones), upper.append((1.0 - p)[:, None] * ones), levels.append(p)
        lower, upper, levels = np.concatenate(lower), np.concatenate(upper), np.concatenate(levels)
        counts = qe.component_concordance(self._quantity, lower, upper, scores=[d[0] for d in densities])
        if int(np.sum(counts.n)) == 0:
            raise Exception("All samples were masked")
        st = qe.concordance_statistics(counts.n, counts.pair)
        return dict(prob=st["prob"], var=st["var"], levels=levels, counts=counts, corr=corr, dof=dof)

    @staticmethod
    def _tail_dependence(walk, dof):
        """TailDependence of a pass of _tail_concordance under the Gaussian (dof None) or the Student-t copula"""
        from scipy import special
        from .tool import simple_distribution
        prob, var, levels, counts, corr = walk["prob"], walk["var"], walk["levels"], walk["counts"], walk["corr"]
        M = corr.shape[0]
        if dof is None:
            h = special.ndtri(levels)
            model = simple_distribution.bivariate_orthant(h[:, None, None], h[:, None, None], np.clip(corr, -1.0, 1.0)[None])
        else:
            h = special.stdtrit(dof, levels)
            model = simple_distribution.bivariate_t_orthant(h[:, None, None], h[:, None, None], np.clip(corr, -1.0, 1.0)[None], dof)
        rest = (1.0 - levels)[:, None, None]
        with np.errstate(all="ignore"):
            z = np.where(np.isfinite(var) & (var > 0.0), (prob - model) / np.sqrt(var), np.nan)
        z[:, np.arange(M), np.arange(M)] = np.nan
        marginal = prob[:, np.arange(M), np.arange(M)].copy()
        return TailDependence(prob, var, prob / rest, model, model / rest, z, marginal, counts, counts.n, counts.n_rm, corr)

    def estimate_copula_dof(self, probs=(0.9, 0.95), tail="both", corr=None, grid=None, densities=None, tol=1e-8, reg_param=0.0,
                            orth_moments_tol=1e-4, moments_fns=None):
        """The degrees of freedom of a Student-t copula for the components, read off the tail concordance of the stored samples:
        ONE pass as in `estimate_tail_dependence` (the counts do not depend on nu), then host arithmetic over a grid of nu
        (tool.simple_distribution.fit_copula_dof): the nu whose t orthants lie closest to the frequencies, np.inf for the Gaussian
        copula.  Feed the result to `sample_joint(dof=...)`, `estimate_aggregates(dof=...)`, `estimate_tail_dependence(dof=...)`
        and to the joint numbers themselves: `estimate_joint_probability(dof=...)`, `estimate_joint_exceedance(dof=...)`,
        `sample_given_event(dof=...)`, `estimate_event_means(dof=...)` and the two bootstrap bands (Genz and Bretz's mixing
        variable), and to the what-if fan: `sample_conditional(dof=...)`, `estimate_conditional_quantiles(dof=...)`,
        `estimate_conditional_probability(dof=...)`, `estimate_conditional_exceedance(dof=...)`, `sample_conditional_event(dof=...)`,
        `estimate_conditional_event_means(dof=...)` and `estimate_conditional_aggregates(dof=...)` (`given` on the joint entries
        themselves conditions under the Gaussian copula only).  Not provided under a t copula: bootstrap bands of conditional
        probabilities, and a bootstrap of nu -- the fit has no error bar beyond the objective's shape over the grid (`estimate_copula_likelihood` fits
        nu from every sample and gives each candidate a paired error bar).
        :param probs, tail, corr, densities: as in estimate_tail_dependence; corr="quadrant" is the estimate that is consistent
            under a t copula
        :param grid: candidate nu, finite values in [1, 64] or np.inf; None: 2, 3, 4, 5, 6, 8, 10, 15, 20, 30, inf
        :return: (CopulaDofFit(dof, grid, objective, z), TailDependence at the fitted nu)"""
        from .tool import simple_distribution
        what = "estimate_copula_dof"
        grid = simple_distribution.COPULA_DOF_GRID if grid is None else grid
        simple_distribution._dof_grid(what, grid)                     # before the pass over the samples
        walk = self._tail_concordance(what, probs, tail, corr, densities, tol, reg_param, orth_moments_tol, moments_fns)
        fit = simple_distribution.fit_copula_dof(walk["prob"], walk["var"], walk["levels"], walk["corr"], grid)
        return fit, self._tail_dependence(walk, None if fit.dof == np.inf else fit.dof)

    def _likelihood_corr_specs(self, what, corr, G):
        """one entry per grid value from `corr` of estimate_copula_likelihood: None, "scores", "quadrant" or a matrix [M, M] for all,
        or a sequence of G such values; checked before any walk"""
        def one(c):
            if c is None:
                return None
            if isinstance(c, str):
                if c not in ("scores", "quadrant"):
                    raise ValueError("{}: corr must be None, 'scores', 'quadrant' or a correlation matrix, got {!r}".format(what, c))
                return c
            m = np.asarray(c, dtype=np.float64)
            if m.ndim != 2 or m.shape[0] != m.shape[1]:
                raise ValueError("{}: corr must be None, 'scores', 'quadrant' or a correlation matrix [M, M], or one such value "
                                 "per grid entry; got an array of shape {}".format(what, m.shape))
            return m
        if corr is None or isinstance(corr, str):
            return [one(corr)] * G
        if isinstance(corr, (list, tuple)) and any(c is None or isinstance(c, str) or np.ndim(c) == 2 for c in corr):
            if len(corr) != G:
                raise ValueError("{}: {} correlations for {} grid values".format(what, len(corr), G))
            return [one(c) for c in corr]
        m = np.asarray(corr, dtype=np.float64)
        if m.ndim == 3:
            if m.shape[0] != G:
                raise ValueError("{}: {} correlations for {} grid values".format(what, m.shape[0], G))
            return [one(c) for c in m]
        return [one(m)] * G

    def estimate_copula_likelihood(self, dofs=None, corr="quadrant", densities=None, tol=1e-8, reg_param=0.0, orth_moments_tol=1e-4,
                                   moments_fns=None):
        """The degrees of freedom of a Student-t copula for the components by PSEUDO-LIKELIHOOD (inference functions for margins):
        the multilevel mean of the copula log density at the probability-integral transforms of the stored samples, for every nu of
        a grid, np.inf being the Gaussian copula.  Unlike `estimate_copula_dof`, which reads a few tail counts of pairs, it uses
        every sample and the whole M-variate law, and it compares two models with an error bar: the paired differences of their log
        densities.  ONE pass over the stored samples for the whole grid: each fine and coarse value goes through its marginal's CDF
        on the device, and mlmc_copula_log_density evaluates all models on the device-resident uniforms
        (quantity_estimate.component_copula_likelihood).
        :param dofs: candidate nu, finite values in [1, 64] or np.inf; None: tool.simple_distribution.COPULA_DOF_GRID
        :param corr: what `estimate_tail_dependence` takes -- None (Pearson), "scores", "quadrant" or a correlation matrix [M, M] --
            or one such value per grid entry, e.g. "scores" for np.inf and "quadrant" for the finite nu ("quadrant" is the estimate
            that is consistent under a t copula, "scores" the efficient one under the Gaussian copula).  Every matrix goes through
            tool.simple_distribution.correlation_factor; the repaired matrix is the one whose density is evaluated
        :param densities: as in estimate_component_quantiles
        :return: (CopulaLikelihood, success).  CopulaLikelihood(dof, grid, loglik, stderr [G], delta, delta_stderr, z [G], l_means,
            l_vars [L, G], n_samples, n_rm_samples [L], corr [G, M, M]):
            loglik = sum over the levels of the mean of l^f - l^c, stderr = sqrt(sum_l var_l / n_l);
            dof = the grid value with the largest loglik, a tie goes to the larger nu (as in fit_copula_dof);
            delta = the paired multilevel difference of every model from the best one (<= 0), delta_stderr its standard error from
            the sums of d_g d_h, z = delta / delta_stderr (0 at the best model, NaN where the standard error is not positive and
            finite); corr the correlation matrices that were evaluated.  success [M]: whether each marginal's fit converged.
        What the error bars do NOT contain: the sampling error of the correlation estimates and of the fitted marginals."""
        from .tool import simple_distribution
        what = "estimate_copula_likelihood"
        grid = simple_distribution._dof_grid(what, simple_distribution.COPULA_DOF_GRID if dofs is None else dofs)
        G = grid.size
        if G > simple_distribution._lib.COPULA_LIK_MAX_G:
            raise ValueError("{}: at most {} grid values per call".format(what, simple_distribution._lib.COPULA_LIK_MAX_G))
        specs = self._likelihood_corr_specs(what, corr, G)
        if isinstance(densities, str):
            raise ValueError(what + ": densities must be the list construct_densities returned")
        if densities is None:
            densities = self.construct_densities(tol, reg_param, orth_moments_tol, moments_fns)
        densities = list(densities)
        M = int(self._quantity.size())
        if len(densities) != M:
            raise ValueError("{}: {} densities for {} components".format(what, len(densities), M))
        success = np.array([bool(d[2].success) for d in densities], dtype=bool)
        named, mats = {}, []
        for spec in specs:
            key = spec if (spec is None or isinstance(spec, str)) else None
            if isinstance(spec, np.ndarray):
                m = spec
            else:
                if key not in named:
                    named[key] = np.asarray(self._copula_correlation(what, spec, densities, tol, reg_param, orth_moments_tol,
                                                                     moments_fns)[0], dtype=np.float64)
                m = named[key]
            if m.shape != (M, M):
                raise ValueError("{}: corr of shape {}, expected ({}, {})".format(what, m.shape, M, M))
            mats.append(m)
        sums = qe.component_copula_likelihood(self._quantity, [d[0] for d in densities], np.stack(mats), grid)
        if int(np.sum(sums.n)) == 0:
            raise Exception("All samples were masked")
        st = simple_distribution.likelihood_statistics(sums.n, sums.sum_diff, sums.sum_gram)
        loglik = st["loglik"]
        best_ll = np.max(loglik)
        ties = np.flatnonzero(loglik == best_ll)
        best = int(ties[np.argmax(grid[ties])]) if ties.size else 0
        with np.errstate(all="ignore"):
            stderr = np.sqrt(st["var"])
            delta = st["delta"][:, best].copy()
            delta_stderr = np.sqrt(st["delta_var"][:, best])
            z = np.where(np.isfinite(delta_stderr) & (delta_stderr > 0.0), delta / delta_stderr, np.nan)
        z[best] = 0.0
        return CopulaLikelihood(float(grid[best]), grid, loglik, stderr, delta, delta_stderr, z, st["l_means"], st["l_vars"],
                                np.asarray(sums.n, dtype=np.int64), np.asarray(sums.n_rm, dtype=np.int64), sums.models.corr), success

    def estimate_quadrant_correlation(self, densities=None, tol=1e-8, reg_param=0.0, orth_moments_tol=1e-4, moments_fns=None):
        """The correlation matrix of the copula from how often two components lie above their medians at once: for every elliptical
        copula -- Gaussian or Student-t with any degrees of freedom -- P(U_a > 1/2, U_b > 1/2) = 1/4 + asin(rho_ab) / (2 pi), so
            rho_ab = sin(2 pi (P_ab - 1/4)),   stderr_ab = 2 pi |cos(2 pi (P_ab - 1/4))| sqrt(var_ab).
        One concordance pass with the single event u > 1/2 (quantity_estimate.component_concordance(scores=...)).
        :param densities: as in estimate_component_quantiles
        :return: QuadrantCorrelation(corr [M, M] clipped to [-1, 1] with a unit diagonal, stderr [M, M] (0 on the diagonal),
            prob, var [M, M] the multilevel frequency and its variance, counts)"""
        what = "estimate_quadrant_correlation"
        if isinstance(densities, str):
            raise ValueError(what + ": densities must be the list construct_densities returned")
        if densities is None:
            densities = self.construct_densities(tol, reg_param, orth_moments_tol, moments_fns)
        densities = list(densities)
        M = int(self._quantity.size())
        if len(densities) != M:
            raise ValueError("{}: {} densities for {} components".format(what, len(densities), M))
        counts = qe.component_concordance(self._quantity, 0.5 * np.ones((1, M)), np.inf * np.ones((1, M)),
                                          scores=[d[0] for d in densities])
        if int(np.sum(counts.n)) == 0:
            raise Exception("All samples were masked")
        st = qe.concordance_statistics(counts.n, counts.pair)
        corr, stderr = quadrant_correlation(st["prob"][0], st["var"][0])
        return QuadrantCorrelation(corr, stderr, st["prob"][0], st["var"][0], counts)

    def estimate_joint_frequency(self, lower, upper):
        """The direct multilevel estimate of P(lower_m < X_m < upper_m for every component m) from the stored samples, in the units
        of the components, for B boxes in one pass (quantity_estimate.component_concordance(pairs=False)): no densities and no
        copula are involved.  This is the number to hold against `estimate_joint_probability(...).prob` at moderate probabilities:
        where the two disagree beyond stderr, the marginals or the copula do not describe the samples.  It CANNOT resolve rare
        events: it counts, so a box of probability P needs of the order of 100 / P samples on the coarsest level for a 10 % error,
        and a box that no stored sample falls into gives exactly 0 with a variance of 0 -- where `estimate_joint_probability`
        integrates the model and resolves 1e-6.  A sample with a NaN in any component, fine or coarse, is dropped.
        :param lower, upper: broadcast to [B, M] ([M]: one box); -inf / +inf: no limit on that side; at most 16 boxes per call
        :return: JointFrequency(prob [B], stderr [B], counts, n_samples [L]): stderr = sqrt(sum_l var_l / n_l), exact from the
            integers (the level difference of an indicator is -1, 0 or 1); counts: quantity_estimate.ComponentConcordance"""
        counts = qe.component_concordance(self._quantity, lower, upper, pairs=False)
        if int(np.sum(counts.n)) == 0:
            raise Exception("All samples were masked")
        st = qe.concordance_statistics(counts.n, counts.all)
        with np.errstate(all="ignore"):
            stderr = np.sqrt(st["var"])
        return JointFrequency(st["prob"], stderr, counts, counts.n)

    def sample_given_event(self, n, lower, upper, seeds=tuple(range(8)), corr=None, given=None, tol=1e-8, reg_param=0.0,
                           orth_moments_tol=1e-4, moments_fns=None, densities=None, first=0, device=False, qmc=True, dof=None,
                           mixing="plain"):
        """Joint scenarios of all components GIVEN that they lie in a box at once (lower_m < X_m < upper_m for all m), under the
        marginals and the Gaussian copula of `sample_joint`, for B events and R seeds (tool.simple_distribution.event_samples):
        what the system looks like when the event of `estimate_joint_probability` happens.  Every scenario lies in the event and
        carries an importance weight, at any probability of the event; filtering the scenarios of `sample_joint` keeps none of
        2^16 at a probability of 1e-6.
        :param n: scenarios per seed and event; a power of two with `first` a multiple of it
        :param lower, upper: broadcast to [B, M] in the components' own units; +-inf does not constrain that side
        :param seeds: one independent scramble each
        :param corr: as in sample_joint: None (Pearson), "scores", or a correlation matrix [M, M] of the normal scores
        :param given: None, or as in sample_conditional: the scenarios are conditional on these values too; a given component
            must not be constrained
        :param densities: as in estimate_component_quantiles
        :param device: the arrays of the result are float64 torch device tensors
        :param dof: None or np.inf: the Gaussian copula, bit for bit; a float in [1, 64]: the Student-t copula of
            `sample_joint(dof=...)`, as in estimate_joint_probability (corr="quadrant" is the consistent correlation).  Not together
            with `given`: that is `sample_conditional_event`
        :param mixing: "plain" (default, bit for bit as before) or "conditioned" (dof only, not with `given`): the component with the
            smallest marginal probability of each box LEADS: it is drawn inside its limits and the mixing scale follows its law given
            that draw (tool.simple_distribution.joint_probabilities / event_samples), so the relative error holds at any depth of
            the box.  Plain mixing returns a number that is orders of magnitude too small, with a `stderr` that does not show it,
            once only a rare mixing scale reaches the box (marginal levels of 1e-6 at dof = 3)
        :return: (EventScenarios(draws [R, B, M, n], weights [R, B, n], prob, ess [R, B], ok [M], uniforms), success [M])"""
        from .tool import simple_distribution
        what = "sample_given_event"
        dof = simple_distribution._box_dof(what, dof, None, given)
        simple_distribution._check_mixing(what, mixing, dof, None, given)
        return self._given_event(what, simple_distribution.event_samples, n, lower, upper, seeds, corr, given, tol, reg_param,
                                 orth_moments_tol, moments_fns, densities, first, device, qmc, dof, mixing)

    def sample_conditional_event(self, n, lower, upper, given, seeds=tuple(range(8)), corr=None, tol=1e-8, reg_param=0.0,
                                 orth_moments_tol=1e-4, moments_fns=None, densities=None, first=0, device=False, qmc=True, dof=None):
        """Joint scenarios of all components GIVEN a box event AND measured or fixed values of some components
        (tool.simple_distribution.conditional_event_samples).  With dof None this is `sample_given_event(given=...)`, bit for bit,
        through the same body; with dof the copula is the Student-t copula, as in estimate_conditional_probability.
        :param given: as in sample_conditional (required); a given component must not be constrained
        :param n, lower, upper, seeds, corr, densities, first, device, qmc: as in sample_given_event
        Like the whole conditional family this keeps PLAIN mixing (see estimate_conditional_probability).
        :return: (EventScenarios, success [M]); rows of given components hold the given values"""
        from .tool import simple_distribution
        what = "sample_conditional_event"
        if given is None:
            raise ValueError(what + ": given is required (without given values: sample_given_event)")
        nu = simple_distribution._check_dof(what, dof)
        simple_distribution._check_conditional_dof(what, nu, len(given) if hasattr(given, "items") else 0)
        return self._given_event(what, simple_distribution.conditional_event_samples, n, lower, upper, seeds, corr, given, tol, reg_param, orth_moments_tol, moments_fns,
                                 densities, first, device, qmc, nu)

    def _given_event(self, what, entry, n, lower, upper, seeds, corr, given, tol, reg_param, orth_moments_tol, moments_fns, densities,
                     first, device, qmc, dof, mixing="plain"):
        """the one body of sample_given_event and sample_conditional_event; dof and mixing checked by the caller"""
        from .tool import simple_distribution
        n, seeds, first = simple_distribution._box_call_args(what, n, seeds, first)
        if np.any(np.isnan(np.asarray(lower, dtype=np.float64))) or np.any(np.isnan(np.asarray(upper, dtype=np.float64))):
            raise ValueError(what + ": a limit is NaN (use -inf / +inf for a side without a limit)")
        corr, densities = self._copula_correlation(what, corr, densities, tol, reg_param, orth_moments_tol, moments_fns)
        if densities is None:
            densities = self.construct_densities(tol, reg_param, orth_moments_tol, moments_fns)
        more = {} if mixing == "plain" else {"mixing": mixing}
        result = entry([d[0] for d in densities], lower, upper, n=n, seeds=[int(s) for s in seeds], corr=corr, given=given, first=first,
                       qmc=qmc, device=device, dof=dof, **more)
        success = np.array([bool(d[2].success) for d in densities], dtype=bool)
        return result, success

    def estimate_event_means(self, lower, upper, n=2 ** 14, seeds=tuple(range(8)), corr=None, given=None, tol=1e-8, reg_param=0.0,
                             orth_moments_tol=1e-4, moments_fns=None, densities=None, first=0, qmc=True, dof=None, mixing="plain"):
        """Expected value of EVERY component given that the components lie in a box at once, E[X | lower < X < upper]: the weighted
        means of the scenarios of `sample_given_event`.  `estimate_event_means(thresholds, np.inf)` is the companion of
        `estimate_joint_exceedance`: the expected state of the system when all thresholds are exceeded.  The weights are smooth on
        the Sobol' points, so the error falls like 1 / n at any probability of the event.
        :param lower, upper, n, seeds, corr, given, densities, first, qmc, dof, mixing: as in sample_given_event
        :return: (EventMeans(mean [B, M], stderr [B, M], prob, ess [R, B]), success [M]): per seed the ratio sum f x / sum f, its
            mean over the seeds and their spread over sqrt(R); prob the JointProbability of the event; ess the effective sample
            size of each seed's n scenarios"""
        scen, success = self.sample_given_event(n, lower, upper, seeds=seeds, corr=corr, given=given, tol=tol, reg_param=reg_param,
                                                orth_moments_tol=orth_moments_tol, moments_fns=moments_fns, densities=densities,
                                                first=first, qmc=qmc, dof=dof, mixing=mixing)
        mean, stderr = scen.means()
        return EventMeans(mean, stderr, scen.prob, scen.ess), success

    def estimate_conditional_event_means(self, lower, upper, given, n=2 ** 14, seeds=tuple(range(8)), corr=None, tol=1e-8, reg_param=0.0,
                                         orth_moments_tol=1e-4, moments_fns=None, densities=None, first=0, qmc=True, dof=None):
        """E[X | lower < X < upper, the given values]: the weighted means of the scenarios of `sample_conditional_event`; with dof
        None `estimate_event_means(given=...)` bit for bit.
        :param lower, upper, given, n, seeds, corr, densities, first, qmc, dof: as in sample_conditional_event
        :return: (EventMeans, success [M])"""
        scen, success = self.sample_conditional_event(n, lower, upper, given, seeds=seeds, corr=corr, tol=tol, reg_param=reg_param,
                                                      orth_moments_tol=orth_moments_tol, moments_fns=moments_fns, densities=densities,
                                                      first=first, qmc=qmc, dof=dof)
        mean, stderr = scen.means()
        return EventMeans(mean, stderr, scen.prob, scen.ess), success

    def estimate_aggregates(self, weights=None, probs=(0.05, 0.5, 0.95), n=2 ** 16, seeds=tuple(range(8)), corr=None, given=None,
                            lower=None, upper=None, members=None, extremes=("max", "min"), event=None, tail="upper", qmc=True,
                            block=2 ** 20, tol=1e-8, reg_param=0.0, orth_moments_tol=1e-4, moments_fns=None, densities=None, first=0,
                            antithetic=False, dof=None, mixing="plain"):
        """The distribution of FUNCTIONS of the components under the marginals and the Gaussian copula of `sample_joint`: the total
        over a field (sum_m w_m X_m), the worst component and which one it is, how many components violate their limits at
        once.  The scenarios are drawn and reduced block by block on the device (tool.simple_distribution.joint_aggregates), so the
        scenario matrix [M, n] never exists; every statistic is formed per seed and the seeds give the error bar.
        The rows: one per row of `weights` ('linear0', ...), then 'max', 'min' (over `members`) as listed in `extremes`, 'count' when
        limits are given, and 'argmax' / 'argmin' next to 'max' / 'min'.  Per seed and row: the quantiles at `probs`
        (np.percentile of the row, bit for bit; with `event` the weighted rule of EventScenarios.weighted_quantiles), mean and
        variance, and the expected shortfall beyond each quantile (tool.simple_distribution.row_statistics with the quantile as
        the threshold; tail 'upper': E[Y | Y >= q_p]).  From the count row count_prob[k] = P(N = k), k = 0 .. M, so count_prob[0] is
        the box probability of `estimate_joint_probability` by counting; from the argmax row worst_prob[m] = P(argmax = m), from the
        argmin row best_prob[m] = P(argmin = m).  Over the seeds: the mean, and the sample standard deviation over sqrt(R) as
        `*_stderr` (NaN for one seed).
        :param weights: None, [M] or [A, M]: the linear rows
        :param probs: probabilities in [0, 1]
        :param n: scenarios per seed, indices first .. first + n - 1; with qmc a power of two with `first` a multiple of it
        :param seeds: one independent replicate each
        :param corr: as in sample_joint: None (Pearson), "scores", or a correlation matrix [M, M] of the normal scores
        :param given: None, or as in sample_conditional: arrays [B] give every result a leading axis B
        :param lower, upper: None or the limits [M] of the count row (-inf / +inf: none on that side)
        :param members: None or a mask [M]: the components the extremes run over
        :param extremes: names among 'max', 'min'
        :param event: None, or (lower_e, upper_e): the scenarios are those of `sample_given_event` for these B boxes and every
            statistic carries their weights; `prob` is the JointProbability of the event.  qmc then chooses Sobol' or Philox points
        :param block: scenario columns per device block
        :param dof: None or np.inf: the Gaussian copula; a float in [1, 64]: the Student-t copula of `sample_joint(dof=...)`, with
            `event` that of `sample_given_event(dof=...)`.  Not together with `given`: that is `estimate_conditional_aggregates`
        :param mixing: with `event` and dof: as in sample_given_event ("conditioned": the conditioned lead); without `event` there is
            no box and "conditioned" raises
        :return: (AggregateSummary, success [M]).  Statistics are [Q, ...], with a leading axis B for arrays in `given` and for the B
            boxes of `event` (always, also for one box); count_prob [.., M + 1], worst_prob / best_prob [.., M] are None without their row"""
        from .tool import simple_distribution as sd
        if sd._check_mixing("estimate_aggregates", mixing, sd._check_dof("estimate_aggregates", dof), None, given) and event is None:
            raise ValueError('estimate_aggregates: mixing="conditioned" needs event (without a box there is no lead component)')
        return self._aggregates("estimate_aggregates", (_refuse_dof_with_given, sd.joint_aggregates, sd.event_samples), weights, probs, n, seeds, corr, given, lower, upper, members, extremes, event, tail, qmc,
                                block, tol, reg_param, orth_moments_tol, moments_fns, densities, first, antithetic, dof, mixing)

    def estimate_conditional_aggregates(self, given, weights=None, probs=(0.05, 0.5, 0.95), n=2 ** 16, seeds=tuple(range(8)), corr=None,
                                        lower=None, upper=None, members=None, extremes=("max", "min"), event=None, tail="upper",
                                        qmc=True, block=2 ** 20, tol=1e-8, reg_param=0.0, orth_moments_tol=1e-4, moments_fns=None,
                                        densities=None, first=0, antithetic=False, dof=None):
        """`estimate_aggregates(given=...)`, the aggregates member of the conditional family, through the same body: with dof None
        bit for bit that call; with dof the scenarios are those of `sample_conditional(dof=...)`
        (tool.simple_distribution.conditional_aggregates) or, with `event`, of `sample_conditional_event(dof=...)`.
        :param given: as in sample_conditional (required); the other arguments as in estimate_aggregates
        :return: (AggregateSummary, success [M])"""
        from .tool import simple_distribution as sd
        what = "estimate_conditional_aggregates"
        if given is None:
            raise ValueError(what + ": given is required (without given values: estimate_aggregates)")
        return self._aggregates(what, (_conditional_dof_with_given, sd.conditional_aggregates, sd.conditional_event_samples), weights, probs, n, seeds, corr, given, lower, upper, members, extremes, event, tail, qmc,
                                block, tol, reg_param, orth_moments_tol, moments_fns, densities, first, antithetic, dof)

    def _aggregates(self, what, entries, weights, probs, n, seeds, corr, given, lower, upper, members, extremes, event, tail, qmc,
                    block, tol, reg_param, orth_moments_tol, moments_fns, densities, first, antithetic, dof, mixing="plain"):
        """the one body of estimate_aggregates and estimate_conditional_aggregates; entries: (the check of dof against given, the
        aggregates entry, the event entry) of tool.simple_distribution"""
        from .tool import simple_distribution as sd
        check_given, aggregates, event_samples = entries
        M = int(self._quantity.size())
        n, seeds, first = sd._box_call_args(what, n, seeds, first)
        sd._sample_flags(what, antithetic, qmc)
        dof = sd._check_dof(what, dof)
        check_given(what, dof, given)
        _check_tail(what, tail)
        probs = np.atleast_1d(np.asarray(probs, dtype=np.float64)).reshape(-1)
        if probs.size == 0 or not np.all((probs >= 0) & (probs <= 1)):
            raise ValueError(what + ": probs must be probabilities in [0, 1], got {}".format(probs.tolist()))
        if isinstance(extremes, str):
            extremes = (extremes,)
        extremes = tuple(extremes)
        if any(name not in ("max", "min") for name in extremes):
            raise ValueError(what + ": extremes must be among 'max', 'min', got {!r}".format(extremes))
        extremes = extremes + tuple("arg" + name for name in extremes)
        agg = dict(weights=weights, lower=lower, upper=upper, members=members, extremes=extremes)
        names = sd._aggregate_args(what, M, **agg)[-1]
        if event is not None:
            if antithetic:
                raise ValueError(what + ": antithetic does not apply to the scenarios of an event")
            try:
                lower_e, upper_e = event
            except (TypeError, ValueError):
                raise ValueError(what + ": event must be a pair (lower, upper) of limits") from None
            if np.any(np.isnan(np.asarray(lower_e, dtype=np.float64))) or np.any(np.isnan(np.asarray(upper_e, dtype=np.float64))):
                raise ValueError(what + ": a limit of the event is NaN (use -inf / +inf for a side without a limit)")
        corr, densities = self._copula_correlation(what, corr, densities, tol, reg_param, orth_moments_tol, moments_fns)
        if densities is None:
            densities = self.construct_densities(tol, reg_param, orth_moments_tol, moments_fns)
        distrs = [d[0] for d in densities]
        success = np.array([bool(d[2].success) for d in densities], dtype=bool)
        Q, K, R = len(names), probs.size, seeds.size
        prob = None
        if event is None:
            per_seed = [aggregates(distrs, n, int(s), corr=corr, given=given, first=first, antithetic=antithetic, qmc=qmc, block=block,
                                   device=True, dof=dof, **agg).rows for s in seeds]
            lead = tuple(per_seed[0].shape[:-2])
            f_of = None
        else:
            scen = event_samples(distrs, lower_e, upper_e, n=n, seeds=[int(s) for s in seeds], corr=corr, given=given, first=first, qmc=qmc,
                                 device=True, dof=dof, **({} if mixing == "plain" else {"mixing": mixing}))
            ev = sd.event_aggregates(scen, **agg)
            B = int(ev.rows.shape[1])
            per_seed = [ev.rows[r] for r in range(R)]
            lead = (B,)
            f_of = ev.weights.cpu().numpy()
            prob = scen.prob
        nB = int(np.prod(lead, dtype=np.int64))
        rep = dict(quantiles=np.empty((R, nB, Q, K)), mean=np.empty((R, nB, Q)), var=np.empty((R, nB, Q)),
                   shortfall=np.empty((R, nB, Q, K)))
        k_count, k_max, k_min = (names.index(s) if s in names else None for s in ("count", "argmax", "argmin"))
        if k_count is not None:
            rep["count_prob"] = np.empty((R, nB, M + 1))
        if k_max is not None:
            rep["worst_prob"] = np.empty((R, nB, M))
        if k_min is not None:
            rep["best_prob"] = np.empty((R, nB, M))

        def masses(stat):                                             # P(Y = k) from P(Y >= k), k = 0 .. len - 1
            return stat.tail_prob - np.append(stat.tail_prob[1:], 0.0)

        for r in range(R):
            rows = per_seed[r].reshape(nB, Q, n)
            for b in range(nB):
                f = None if f_of is None else f_of[r, b]
                if f is None:
                    q = engine.row_percentiles(rows[b], 100.0 * probs, nan_policy="propagate")
                else:
                    q = _weighted_row_quantiles(rows[b].cpu().numpy(), f, probs)
                ok = np.all(np.isfinite(q), axis=1)
                st = sd.row_statistics(rows[b], f=f, thresholds=np.where(ok[:, None], q, 0.0), tail=tail)
                rep["quantiles"][r, b], rep["mean"][r, b], rep["var"][r, b] = q, st.mean, st.var
                rep["shortfall"][r, b] = np.where(ok[:, None], st.tail_mean, np.nan)
                for key, k_row, size in (("count_prob", k_count, M + 1), ("worst_prob", k_max, M), ("best_prob", k_min, M)):
                    if k_row is not None:
                        rep[key][r, b] = masses(sd.row_statistics(rows[b, k_row], f=f, thresholds=np.arange(size, dtype=np.float64)))
        out = {}
        for key in ("quantiles", "mean", "var", "shortfall", "count_prob", "worst_prob", "best_prob"):
            if key not in rep:
                out[key] = out[key + "_stderr"] = None
                continue
            v = rep[key]
            shape = lead + v.shape[2:]
            with np.errstate(invalid="ignore"):
                out[key] = v.mean(axis=0).reshape(shape)
                out[key + "_stderr"] = (np.std(v, axis=0, ddof=1) / np.sqrt(R) if R > 1 else np.full(v.shape[1:], np.nan)).reshape(shape)
        return AggregateSummary(names=names, probs=probs, prob=prob, n=n, seeds=seeds, **out), success

    def estimate_conditional_quantiles(self, probs, given, corr=None, tol=1e-8, reg_param=0.0, orth_moments_tol=1e-4, moments_fns=None,
                                       densities=None, dof=None):
        """Quantiles of every component that is not in `given`, conditional on the given values of the others
        (tool.simple_distribution.conditional_quantiles): medians and bands of the rest of the vector once some of it is known.
        :param probs: probabilities, the same for every component
        :param given, corr, densities, dof: as in sample_conditional
        :return: (q, success): q [q, len(probs)] for scalar values, [B, q, len(probs)] for arrays, row m = the m-th component
            that is not given, ascending; success [M] bool, the solver's verdict per component"""
        from .tool import simple_distribution
        nu = simple_distribution._check_dof("estimate_conditional_quantiles", dof)
        simple_distribution._check_conditional_dof("estimate_conditional_quantiles", nu, len(given) if hasattr(given, "items") else 0)
        corr, densities = self._copula_correlation("estimate_conditional_quantiles", corr, densities, tol, reg_param,
                                                   orth_moments_tol, moments_fns)
        if densities is None:
            densities = self.construct_densities(tol, reg_param, orth_moments_tol, moments_fns)
        q = simple_distribution.conditional_quantiles([d[0] for d in densities], probs, given, corr, dof=dof)
        success = np.array([bool(d[2].success) for d in densities], dtype=bool)
        return q, success

    def estimate_component_shortfall(self, probs, tail="upper", tol=1e-8, reg_param=0.0, orth_moments_tol=1e-4, moments_fns=None,
                                     densities=None):
        """Expected shortfall (CVaR) of the maximum-entropy density of EVERY scalar component of the quantity, in one batched
        device call (tool.simple_distribution.tail_means): E[X | X >= Q(p)] for tail = "upper", E[X | X <= Q(p)] for "lower".

        :param probs: probabilities, the same for every component
        :param densities: as in estimate_component_quantiles
        :return: (es, q, success): es [M, len(probs)] the shortfall of component m at every level, q [M, len(probs)] the
            quantiles they start from (bit for bit estimate_component_quantiles'), success [M] bool the solver's verdict"""
        from .tool import simple_distribution
        _check_tail("estimate_component_shortfall", tail)
        if densities is None:
            densities = self.construct_densities(tol, reg_param, orth_moments_tol, moments_fns)
        probs = np.atleast_1d(np.asarray(probs, dtype=np.float64)).reshape(-1)
        q, lower, upper, _ = simple_distribution.tail_means([d[0] for d in densities], probs)
        success = np.array([bool(d[2].success) for d in densities], dtype=bool)
        shape = (len(densities), probs.size)
        es = np.array(upper if tail == "upper" else lower, dtype=np.float64).reshape(shape)
        return es, np.array(q, dtype=np.float64).reshape(shape), success

    def estimate_component_summaries(self, tol=1e-8, reg_param=0.0, orth_moments_tol=1e-4, moments_fns=None, densities=None):
        """Mean, variance, skewness, kurtosis, differential entropy and mass of the maximum-entropy density of EVERY scalar
        component of the quantity, from two batched device calls (tool.simple_distribution.summaries).
        :param densities: as in estimate_component_quantiles
        :return: DensitySummary(mean, var, skewness, kurtosis, entropy, mass) of [M] arrays, entry m = `.summary()` of component
            m's distribution (the row order of construct_densities); components of failed solves are still returned"""
        from .tool import simple_distribution
        if densities is None:
            densities = self.construct_densities(tol, reg_param, orth_moments_tol, moments_fns)
        return simple_distribution.summaries([d[0] for d in densities])

    def get_level_samples(self, level_id, n_samples=None):
        chunk_spec = next(self._sample_storage.chunks(level_id=level_id, n_samples=n_samples))
        return self._quantity.samples(chunk_spec=chunk_spec)


def scalar_component(quantity, m):
    """Scalar sub-quantity of row m of `quantity.samples(chunk)` ([M, n, 2] -> [1, n, 2]), lowerable to the device like
    any item selection."""
    from .quantity.quantity import Quantity
    from .quantity import quantity_types as qt
    qtype = quantity.qtype
    if isinstance(qtype, qt.ArrayType) and isinstance(qtype._qtype, ScalarType):
        key = tuple(int(i) for i in np.unravel_index(m, qtype._shape))     # ArrayType indexes its shaped rows
    elif isinstance(qtype, qt.ArrayType):
        key = None
    else:
        key = slice(m, m + 1)                                              # the other types index the flat rows
    if key is None:
        item = Quantity(quantity_type=ScalarType(), input_quantities=[quantity], operation=lambda y, m=m: y[m:m + 1])
    else:
        item = Quantity(quantity_type=ScalarType(), input_quantities=[quantity],
                        operation=lambda y, key=key: qtype._make_getitem_op(y, key=key))
        item._sym = ("getitem", key)
    return item


def estimate_domain(quantity, sample_storage, quantile=None):
    """Module-level variant (reference: :344-363): percentile range of the fine samples of every level -- the first
    n_collected[0] samples of each (`ChunkSpec(level_id, n_samples=n_collected()[0])`), NaNs not removed (np.percentile
    then yields NaN, :360).  The samples stay where the device wants them (quantity_estimate.fine_samples_for_device)."""
    if quantile is None:
        quantile = 0.01
    ranges = []
    for level_id in range(sample_storage.get_n_levels()):
        n0 = sample_storage.get_n_collected()[0]
        chunk_spec = next(sample_storage.chunks(level_id=level_id, n_samples=n0))
        fine = qe.fine_samples_for_device(quantity, chunk_spec)
        ranges.append(engine.percentiles(fine, [100 * quantile, 100 * (1 - quantile)], nan_policy="propagate"))
    ranges = np.array(ranges)
    return np.min(ranges[:, 0]), np.max(ranges[:, 1])


def estimate_domains(quantity, sample_storage, quantile=None):
    """-> [M, 2]: row m is estimate_domain(scalar_component(quantity, m), sample_storage, quantile), bit for bit: the same
    chunks, one device call per level for all components, a NaN in a component's samples of some level gives that component
    [nan, nan]."""
    if quantile is None:
        quantile = 0.01
    n_comp = int(quantity.size())
    ranges = []
    for level_id in range(sample_storage.get_n_levels()):
        n0 = sample_storage.get_n_collected()[0]
        chunk_spec = next(sample_storage.chunks(level_id=level_id, n_samples=n0))
        fine = qe.fine_samples_for_device(quantity, chunk_spec)
        ranges.append(engine.row_percentiles(fine.reshape(n_comp, -1), [100 * quantile, 100 * (1 - quantile)],
                                             nan_policy="propagate"))
    return _domains_of(ranges)


def _domains_of(ranges):
    """[L] of [M, 2] per-level percentile pairs -> [M, 2]: min of the lower, max of the upper over the levels (np.min /
    np.max as estimate_domain takes them: a NaN propagates)."""
    ranges = np.array(ranges)                    # [L, M, 2]
    return np.stack((np.min(ranges[:, :, 0], axis=0), np.max(ranges[:, :, 1], axis=0)), axis=1)


def estimate_n_samples_for_target_variance(target_variance, prescribe_vars, n_ops, n_levels):
    """Optimal samples per level for a target variance of every moment (reference: :366-385).

    n_l = round( sqrt(V_l / C_l) * sum_k sqrt(V_k C_k) / target ), capped by V_l L / target, at least 2; max over moments.
    :return: int array [L]"""
    variances = np.asarray(prescribe_vars, dtype=np.float64)
    n_ops = np.asarray(n_ops, dtype=np.float64)
    sqrt_var_cost = np.sqrt(variances.T * n_ops)                    # [R, L]
    total = np.sum(sqrt_var_cost, axis=1)                           # [R]
    n_est = np.round((sqrt_var_cost / n_ops).T * total / target_variance).astype(int)     # [L, R]
    n_safe = np.maximum(np.minimum(n_est, variances * n_levels / target_variance), 2)
    return np.max(n_safe, axis=1).astype(int)


def _geometric_level_params(step_range, n_levels):
    assert step_range[0] > step_range[1]
    params = []
    for i in range(n_levels):
        frac = 1 if n_levels == 1 else i / (n_levels - 1)
        params.append([step_range[0] ** (1 - frac) * step_range[1] ** frac])
    return params


def calc_level_params(step_range, n_levels):
    """Geometric sequence of level steps (reference: :388-398)."""
    return _geometric_level_params(step_range, n_levels)


def determine_level_parameters(n_levels, step_range):
    """Geometric sequence of level steps (reference: :409-426)."""
    return _geometric_level_params(step_range, n_levels)


def determine_sample_vec(n_collected_samples, n_levels, sample_vector=None):
    """(reference: :401-406)"""
    if sample_vector is None:
        sample_vector = n_collected_samples
    if len(sample_vector) > n_levels:
        sample_vector = sample_vector[:n_levels]
    return np.array(sample_vector)


def determine_n_samples(n_levels, n_samples=None):
    """Initial number of samples per level: geometric interpolation between n0 and nL (reference: :429-450)."""
    if n_samples is None:
        n_samples = [100, 3]
    n_samples = np.atleast_1d(n_samples)
    if len(n_samples) == 1:
        n_samples = np.array([n_samples[0], 3])
    if len(n_samples) == 2:
        n0, n_last = n_samples
        n_samples = np.round(np.exp2(np.linspace(np.log2(n0), np.log2(n_last), n_levels))).astype(int)
    return n_samples
