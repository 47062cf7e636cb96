#!/usr/bin/env python3
"""Batched CDFs and quantiles of max-entropy densities against what exists without them.

few-points regime: M in {16, 64, 256, 1024} densities of R = 25 moments (Gaussian mixtures of varying shape, solved in one batch),
probs = (0.05, 0.5, 0.95) and linspace(0.01, 0.99, 99):
  quantiles_ms   simple_distribution.quantiles (one mlmc_density_quantiles_batch)
  brentq_ms      scipy.optimize.brentq on d.cdf per (component, probability) at xtol = 4 spacing, TIMED ON A SUBSET of at most
                 8 components x 3 probabilities AND SCALED to M x n_p
  cdfs_ms        simple_distribution.cdfs at the quantiles (one mlmc_density_integrate_batch)
  cdf_loop_ms    the loop [d.cdf(v) for d in distrs]
many-points regime: B in {1, 8, 64} problems x n in {10^6, 10^7} device-resident uniforms, R1 in {9, 25, 64}:
  kernel_ms      HIP-event time of the quantile kernel alone (mlmc_density_quantiles_kernel_time)
  call_ms        wall time of one mlmc_density_quantiles_batch with p and out in device memory: host set-up, upload of the problem
                 table, the two table kernels, the quantile kernel and the wait
  steps          mean evaluations of g per point.  NOT counted on the device: counted by the plain-fp64 twin of the algorithm
                 (tests/quantile_cases.py, same iteration and stopping rules) on 2000 of problem 0's uniforms
  fp64_fraction  steps x gauss_degree x (2 R1 + EXP_FLOPS) x points / kernel_ms against the 78.6 TFLOP/s fp64 vector peak
(--config B,R1,n runs one many-points configuration, e.g. under rocprofv3 --kernel-trace --stats.)
--tails: simple_distribution.tail_means against simple_distribution.quantiles, alternating in one process,
on the same M in {16, 256, 1024} solved densities at 3 and 99 probabilities:
  tail_means_ms / quantiles_ms   wall time of the one device call each
  quad_ms_scaled                 what exists without the entry: scipy.integrate.quad of x density(x) and of density(x) from
                                 d.quantile(p) to the domain end per (component, probability), TIMED ON A SUBSET of at most
                                 4 components x 3 probabilities AND SCALED to M x n_p
and on B = 1, R1 = 25, n = 10^6 device-resident probabilities (--config B,R1,n with --tails: that configuration alone):
  tails_kernel_ms / quantile_kernel_ms   HIP-event time of the point kernels of one call (mlmc_density_quantiles_kernel_time)
  tails_call_ms / quantile_call_ms       wall time of the C entry
--single: the single entries through the C ABI on one solved density of R1 = 25, wall ms of one call up to and including its own wait:
  eval_host_ms / eval_device_ms   mlmc_density_eval at n = 10^3, 10^6, 10^7 host points / n = 10^6 device-resident points
  integrate_ms                    mlmc_density_integrate at n = 10^3, 10^6 host intervals, degree 21
--divergences: simple_distribution.divergences at R1 = 25 on the 64 x 21 rule for P = 16 (16 x 1), 3600
(300 x 12) and 19200 (300 x 64) pairs of n_rep solved replicate densities against n_comp solved priors, the three taking turns:
  divergences_ms      wall time of the one call (problem table of n_comp + P distributions, one mlmc_density_divergences_batch)
  host_sums_ms        (a) the best host alternative of the same definition: ONE simple_distribution.densities call for the
                      n_comp + P distributions at the rule's nodes, then the six sums in NumPy (d from the logarithms)
  quad_ms_scaled      (b) what the public API offers without the entry: KL_divergence and L2_distance with scipy.integrate.quad
                      on d.density, TIMED ON 4 PAIRS AND SCALED to P
  host_vs_entry / quad_vs_entry   largest difference between the alternatives' kl / l2 and the entry's, relative to the value
--moments: simple_distribution.density_moments at R1 = 25, K = 25 (every density's own Legendre basis) on the
64 x 21 rule for B = 16, 3600 and 19200 solved densities, against the host route of the same definition, the two taking turns after
a warm-up call each:
  moments_ms          wall time of the one call (one mlmc_density_moments_batch), [min, mean, max] over the repetitions
  host_sums_ms        ONE simple_distribution.densities call for the B distributions at the rule's nodes, then NumPy: the Legendre
                      functions at the nodes (once: the densities share their basis), the moment sums as one matrix product, the
                      mass and the entropy from the logarithm of the density; [min, mean, max]
  summaries_ms        wall time of simple_distribution.summaries (two calls of the entry and 2 B moments objects), [min, mean, max]
  host_vs_entry       largest difference between the host route's normalised moments and the entry's, absolute
--samples: simple_distribution.samples(..., device=True) against the route that exists without it,
torch.rand on the device + simple_distribution.quantiles, on the same solved densities, the two taking turns after a warm-up call
each; B x R1 x n = 1 x {9, 25, 64} x 10^7, 64 x 25 x 10^6 and 3600 x 25 x 10^3 draws (--config B,R1,n with --samples: that shape alone):
  samples_ms / rand_quantiles_ms                wall time of the whole route up to a device synchronise, [min, mean, max]
  samples_kernel_ms / quantiles_kernel_ms       HIP-event time of the point kernel of one call (mlmc_density_quantiles_kernel_time):
                                                k_q_sample, which makes its uniforms, and k_q_quantile, which reads torch's
  speedup_wall / speedup_kernel                 the route without the entry over the entry, from the means
  ks_samples / ks_rand_quantiles                Kolmogorov distance of the first 10^5 draws of problem 0 (or all its draws) from
                                                cdfs_on_rule, a sanity check of both routes
--joint: simple_distribution.joint_samples(..., device=True) against (a) samples (independent draws) at
the same shape and (b) the route without the entry: torch.randn, torch.matmul with the factor, torch.special.ndtr and
simple_distribution.quantiles on the device uniforms; the three take turns after a warm-up call each; M x R1 x n = 12 x 25 x 10^6,
64 x 25 x 10^6, 256 x 25 x 10^5 with K = M, and 12 x 25 x 10^6 with K = 3 (--config M,R1,n,K with --joint: that shape alone):
  joint_ms / samples_ms / torch_quantiles_ms    wall time of the whole route up to a device synchronise, [min, mean, max]
  joint_kernel_ms / samples_kernel_ms / quantiles_kernel_ms   HIP-event time of one call's point kernels (the joint entry's normals,
                                                uniforms and sampling kernels together; torch's kernels are not in the third)
  joint_over_samples_wall / torch_over_joint_wall   ratios of the mean wall times
--scores: normal_scores(device=True) of n (fine, coarse) pairs of M components (mlmc_density_scores_batch) against cdfs_on_rule on fine
and on coarse followed by torch clamp and torch.special.ndtri, the routes taking turns in one process, for M x R1 x n = 12 x 25 x 10^6,
64 x 25 x 10^6, 256 x 25 x 10^5 (--config M,R1,n,levels with --scores: that shape alone):
  scores_ms / cdf_ndtri_ms                      wall time of the whole route up to a device synchronise, [min, mean, max]
  scores_kernel_ms / cdf_kernel_ms              HIP-event time of one route's point kernels (k_q_scores; the two k_q_cdf launches)
  score_correlation_ms / component_covariance_ms   levels > 0: Estimate.estimate_score_correlation against estimate_component_covariance
                                                on a DeviceMemory store of `levels` levels of n pairs, end to end, mean wall time
--conditional: simple_distribution.conditional_samples(..., device=True) with component 0 of M = 12 given,
R1 = 25, for (B, n) = (1, 10^6), (64, 10^4), (1024, 10^3) against a Python loop of B single-set calls and against joint_samples of the
11 other components with B n draws, the three taking turns after a warm-up call each (--config M,R1,B,n: that shape alone):
  conditional_ms / loop_ms / joint_ms           wall time of the whole route up to a device synchronise, [min, median, max]
  conditional_kernel_ms / loop_kernel_ms / joint_kernel_ms   HIP-event time of one route's point kernels (normals, uniforms, sampling)
  loop_over_conditional_wall / conditional_over_joint_wall   ratios of the median wall times
--tcopula: simple_distribution.joint_samples(..., dof=nu, device=True), the Student-t copula, against the
same call without dof (the Gaussian entry) on the shapes of --joint with K = M, nu = 3 and 30, the two taking turns in one process
after a warm-up each, five repetitions:
  t_ms / gauss_ms                   wall time of the whole route up to a device synchronise, [min, mean, max]
  t_kernel_ms / gauss_kernel_ms     HIP-event time of one call's point kernels (mixing, normals, product, map, sampling)
  map_entry_ms / mixing_entry_ms    wall time of student_t_cdf on M n device values of the t law and of chi2_mixing_scale on n device
                                    uniforms: the map and the mixing kernel on their own, with the entry's launch and wait
  t_over_gauss_wall / t_over_gauss_kernel   ratios of the means
--tconditional: simple_distribution.conditional_samples(..., dof=nu, device=True), component 0 of M given in
B sets, against the same call without dof on the shapes of --conditional, nu = 3 and 30, the two taking turns in one process after a
warm-up each, five repetitions; the keys of --tcopula, with map_entry_ms on B (M - 1) n values and mixing_entry_ms
(conditional_mixing_scale) on n uniforms at nu + 1 degrees of freedom
--qmc: (a) samples, joint_samples and conditional_samples (device=True) with and without qmc=True on the
shapes of --samples, --joint and --conditional (streams = index mod 1024 for both variants), the two taking turns after a warm-up
call each:
  philox_ms / qmc_ms, philox_kernel_ms / qmc_kernel_ms   wall time up to a device synchronise and HIP-event time of the call's point
                                                kernels, [min, median, max]; qmc_over_philox_wall / _kernel the ratios of the medians
(b) the RMS error over seeds 1 .. 8 of the mean of g(u) from joint_samples for n = 2^10, 2^12, .. 2^20 with and without qmc:
g = prod_m (1 + 0.8 (u_m - 1/2)) under M = K = 4, F = I, and g = u_0 u_1 under the 3 x 3 correlation of the tests
--boxprob: copula_box_probabilities of B copies of the box (t, inf)^M under equicorrelation 1/2 with 8
seeds per call (t = 0: the orthant, exactly 1 / (M + 1); for M = 12 also the t at which the probability is 1e-6, against a
one-dimensional quadrature), M = 2 / 12 / 64, B = 1 / 64, n = 2^12 .. 2^20 (--config M,B,n: one orthant shape):
  call_ms, rel_rms             wall time of the call and the RMS over the seeds of a seed's relative error
  count_ms_per_seed, count_rel_rms, count_zero_seeds   the counting route at the same n: joint_samples(device=True), the comparison
                               of the copula uniforms with Phi(t) and the mean in torch, one call per seed
--boxdraws: event_samples(device=True) of the event "components 0 and 1 exceed their 0.9-quantile" (for
M = 12 also their 0.999-quantile) under equicorrelation 1/2 with 8 seeds per call, M = 2 / 12 / 64, n = 2^12 .. 2^20 (--config M,n:
one shape), next to rejection: joint_samples(device=True) of the same n per seed and a filter in torch:
  call_ms, inside_per_ms, ess_fraction, event_mean, event_stderr   wall time of the call up to a device synchronise, its R n scenarios
                               per ms, ess / n, and the conditional mean of component 2 (M = 2: 0) with the seeds' standard error
  reject_ms_per_seed, reject_inside_per_ms, reject_mean, reject_stderr, reject_zero_seeds   the same for what the filter keeps
--tboxprob: the Student-t copula in the two routes above, nu = 3 and 30, against the Gaussian call of the same
shape in the same run, the two taking turns after a warm-up each: copula_box_probabilities(dof=nu) on the shapes of --boxprob (the same
numbers as limits in t-score space), then event_samples(dof=nu, device=True) on the shapes of --boxdraws (--config M,n: one shape of each
with B = 1):
  t_ms / gauss_ms, t_over_gauss_wall   wall time of the call, [min, mean, max], and the ratio of the means
  mixing_entry_ms, map_entry_ms        chi2_mixing_scale on the call's R n device uniforms and (draws) student_t_cdf on its R M n device
                                       scores: the mixing kernel and the CDF pass on their own, with the entry's launch and wait
  prob, stderr / gauss_prob, gauss_stderr (draws: ess_fraction)   what the two calls returned
--tcondbox: the conditional law of the t copula given p = 1 component (dof_mix = nu + 1, a shift and a scale
per box) against the t call of the same shape in the same run, the two taking turns after a warm-up each: conditional_box_probabilities
against copula_box_probabilities(dof=nu) on the shapes of --tboxprob with B in {1, 64} sets of given values, then conditional_box_draws
against copula_box_draws(dof=nu) on the M, n of its draws (--config M,n: one shape of each with B = 1):
  cond_ms / t_ms, cond_over_t_wall   wall time of the call, [min, mean, max], and the ratio of the means
  cond_mixing_entry_ms / t_mixing_entry_ms   the mixing kernel of either call on its own: conditional_mixing_scale(nu + 1) and
                                     chi2_mixing_scale(nu) on the call's R n device uniforms, with the entry's launch and wait
  prob, stderr / t_prob, t_stderr    what the two calls returned for box 0
--tlead: copula_box_probabilities(dof=nu, mixing="conditioned") against the plain t call of the same shape in
the same run, the two taking turns after a warm-up each, on the probability shapes of --tboxprob (B in {1, 64}, nu = 3 and 30; --config
M,n: one shape with B = 1):
  lead_ms / plain_ms, lead_over_plain_wall   wall time of the call, [min, mean, max], and the ratio of the means
  prob, stderr, ess_fraction / plain_prob, plain_stderr, plain_ess_fraction   what the two calls returned for box 0; ess / n from the
                                     integrand of box 0 alone (a call of its own, not timed), the mean over the seeds
--aggregates: mlmc_scenario_aggregates on device-resident scenarios x [S, M, n], A = 3 linear rows, all four
extremes and the count (Q = 8), for S x M x n = 1 x 12 x 10^6, 1 x 64 x 10^6 and 64 given-sets x 12 x 10^4 (--config S,M,n: that shape
alone), against the torch composition on the same materialised matrix -- matmul, max and min with their indices, compare and sum: five
passes over x -- in the same process, the two taking turns after a warm-up call each:
  entry_ms / torch_ms, torch_over_entry_wall   wall time of the whole route up to a device synchronise, and the ratio
  event_ms, tbytes_per_s, fraction_of_stream_rate   HIP-event time around the entry on its stream (one small upload and the one
                               kernel), the algorithmic bytes 8 M n read + 8 Q n written per set over it, and that rate over the
                               5.4 TB/s of this package's own streaming kernels
  extras_equal_torch, linear_rel_diff_torch    the extreme and count rows equal torch's exactly; the linear rows differ from matmul by
                               its summation order
--concordance: concordance_counts(..., device=True) on device-resident uniforms [M, n] with a coarse array and
G = 3 events (u > 0.9, 0.95, 0.99), for M x n = 12 x 10^6, 64 x 10^6 and 256 x 10^5 (--config M,n: that shape alone), against the torch
composition of the same counters -- the keep mask, the fp64 indicator matrices and three fp64 matmul Grams per event -- in the same
process, the two taking turns after a warm-up call each (five repetitions unless --reps says otherwise):
  entry_ms / torch_ms {min, mean, max}, torch_over_entry_wall   wall time of the whole route up to a device synchronise; the ratio of
                               the means
  bits_kernel_ms, gram_kernel_ms   HIP-event time of the streaming kernel and of the Gram kernel (median over the repetitions)
  tbytes_per_s, fraction_of_hbm_peak   16 M n bytes, the one read of the inputs, over the time of the two kernels together, and that
                               rate over the 8 TB/s of the data sheet
  equal_torch                  every counter equals the composition's (exact while counts stay below 2^53)
--loglik: copula_log_density(..., device=True) on device-resident uniforms [M, n] with a coarse array at
equicorrelation 1/2, for M x n = 12 x 10^6 and 64 x 10^5 (--config M,n: that shape alone), once with the default grid of nu (G = 11)
and once with the Gaussian model alone (G = 1), the routes of a shape taking turns after a warm-up call each:
  entry_ms                     wall time of the call up to a device synchronise (the factors of the models are made on the host inside)
  t_quantile_alone_ms, t_quantile_gvalues_per_s   student_t_quantile(nu = 3) on the M n device values of the fine side, and its rate
  host_columns, host_ms_measured, host_ms_extrapolated_to_n, host_over_entry   the host composition of t_scores (SciPy's ndtri and
                               stdtrit) with NumPy on the first host_columns columns of the same uniforms, its time scaled to n
                               columns (the composition is linear in n; the whole of it would take minutes), and that over entry_ms
  torch_ms, torch_over_entry   G = 1 only: torch.special.ndtri + torch.linalg.solve_triangular + the two sums, on the device
  max_abs_difference_from_host / _from_torch   the largest difference of a log density from the composition's
--boxorder: boxes under equicorrelation 1/2 whose lower limits rise from -2 to 2.5 over the components, each
box rotated by its index; the routes of a shape taking turns after a warm-up call each:
  boxorder_kernel   order_ms: box_order alone (upload, the order kernel, download, one wait) for M = 12 / 64 / 128 and B = 1 / 64 / 300
  boxorder_call     ordered_ms: box_order followed by copula_box_probabilities with one factor per box; natural_ms: the call with one
                    shared factor in the caller's order; prob / stderr and natural_prob / natural_stderr of box 0
  boxorder_bands    one_call_ms: joint_probabilities_over_correlations over 301 correlation matrices at M = 12; loop_ms: the loop of 301
                    joint_probabilities calls that it replaces; bit_identical: every replicate of the two is the same
Prints one JSON line.  Usage: python tools/quantile_batch.py [--quick | --config B,R1,n | --single]
                                                             [--tails | --divergences | --moments | --samples | --joint | --tcopula | --tconditional | --scores |
                                                              --conditional | --qmc | --boxprob | --boxdraws | --tboxprob | --tcondbox | --tlead | --aggregates |
                                                              --concordance | --loglik | --boxorder] [--reps K]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from scipy.integrate import quad
from scipy.optimize import brentq

from mlmc_amd import _lib, Legendre
from mlmc_amd.tool import simple_distribution as sd

DOM = (-5.0, 5.0)
PEAK_FP64 = 78.6e12
EXP_FLOPS = 20            # fp64 operations counted for one exp (the library routine's polynomial and range reduction)


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) * 1e3 / reps, out


def mixtures(M, R, seed=11):
    """M solved SimpleDistributions of R moments: two-Gaussian mixtures of varying shape on DOM"""
    fn = Legendre(R, DOM)
    pts, w = sd._composite_gauss(DOM, 256, 21)
    phi = fn.eval_all(pts)
    rng = np.random.default_rng(seed)
    norm = lambda x, m, s: np.exp(-0.5 * ((x - m) / s) ** 2) / (s * np.sqrt(2 * np.pi))
    distrs = []
    for _ in range(M):
        m1, m2 = rng.uniform(-1.2, 1.2, size=2)
        s1, s2 = rng.uniform(0.7, 1.3, size=2)
        p = rng.uniform(0.2, 0.8)
        mom = (p * norm(pts, m1, s1) + (1 - p) * norm(pts, m2, s2)) * w @ phi
        distrs.append(sd.SimpleDistribution(fn, np.stack([mom, np.ones(R)], axis=1), domain=DOM))
    res = sd.estimate_densities_minimize(distrs, tol=1e-8)
    return distrs, all(r.success for r in res)


def few_points(M, probs, reps):
    distrs, ok = mixtures(M, 25)
    q_ms, q = timed(lambda: sd.quantiles(distrs, probs), reps)
    c_ms, _ = timed(lambda: sd.cdfs(distrs, q), reps)
    loop_ms, _ = timed(lambda: [d.cdf(v) for d, v in zip(distrs, q)], 1)
    sub_d, sub_p = distrs[:8], probs[np.linspace(0, len(probs) - 1, 3).astype(int)]
    t0 = time.perf_counter()
    worst = 0.0
    for d, qd in zip(sub_d, q):
        for p in sub_p:
            x = brentq(lambda v: d.cdf(v)[0] - p, DOM[0], DOM[1], xtol=4 * np.spacing(DOM[1]))
            worst = max(worst, abs(x - qd[np.argmin(np.abs(probs - p))]))
    sub_ms = (time.perf_counter() - t0) * 1e3
    brent_ms = sub_ms / (len(sub_d) * len(sub_p)) * M * len(probs)
    return dict(M=M, n_p=len(probs), quantiles_ms=round(q_ms, 3), brentq_ms_scaled=round(brent_ms, 1),
                brentq_subset=[len(sub_d), len(sub_p)], cdfs_ms=round(c_ms, 3), cdf_loop_ms=round(loop_ms, 3),
                brentq_vs_quantiles_dx=float(worst), all_success=ok)


def twin_steps(d, p):
    """mean evaluations of g per point of the bracketed Newton iteration, counted on the fp64 twin of the kernel"""
    from tests import maxent_exact as mx
    from tests import maxent_cases as mc
    from tests import quantile_cases as qc
    desc = mx.Desc(mx.LEGENDRE, d.moments_fn.size, d.domain)
    case = mc.Case("tool", desc, d.moment_means, d._moment_errs, d.multipliers, "tool")
    stats = {}
    qc.twin_quantiles(case, d.multipliers, (d.n_intervals, d._gauss_degree), p, stats)
    return stats["evaluations"] / len(p)


def many_points(B, R1, n, reps):
    distrs, ok = mixtures(B, R1, seed=5)
    g = torch.Generator(device="cuda")
    g.manual_seed(B * 131 + R1)
    flat = torch.rand(B * n, dtype=torch.float64, device="cuda", generator=g)      # problem b: flat[b n : (b + 1) n]
    out = torch.empty_like(flat)
    torch.cuda.synchronize()
    handles, r1, lam, sig = sd._batch_problem_args(distrs)
    a, b = np.full(B, DOM[0]), np.full(B, DOM[1])
    cnt = np.full(B, n, dtype=np.int64)
    n_int, deg = distrs[0].n_intervals, distrs[0]._gauss_degree
    lib, P = _lib.lib(), _lib.ptr

    def call():
        _lib.check(lib.mlmc_density_quantiles_batch(B, C.cast(handles, C.c_void_p), P(r1), P(lam), P(sig), P(a), P(b), n_int, deg,
                                                    P(flat), P(cnt), P(out), None, _lib.DEVICE))
    call()
    k_ms, k_n = C.c_double(), C.c_int64()
    _lib.check(lib.mlmc_density_quantiles_kernel_time(C.byref(k_ms), C.byref(k_n)))           # reset
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    call_ms = (time.perf_counter() - t0) * 1e3 / reps
    _lib.check(lib.mlmc_density_quantiles_kernel_time(C.byref(k_ms), C.byref(k_n)))
    kernel_ms = k_ms.value / k_n.value
    res = out[:n].cpu().numpy()
    mono = bool(np.all(np.diff(res[np.argsort(flat[:n].cpu().numpy())]) >= 0))
    steps = twin_steps(distrs[0], flat[:2000].cpu().numpy())
    flops = steps * deg * (2 * R1 + EXP_FLOPS) * float(B) * n
    return dict(B=B, R1=R1, n=n, kernel_ms=round(kernel_ms, 3), call_ms=round(call_ms, 3), ns_per_point=round(kernel_ms * 1e6 / (B * n), 3),
                steps=round(steps, 2), fp64_fraction=round(flops / (kernel_ms * 1e-3) / PEAK_FP64, 4), monotone=mono, all_success=ok)


def alternating(fns, reps):
    """wall ms per call of every function after one warm-up call each, the functions taking turns inside every repetition"""
    for fn in fns:
        fn()
    total = [0.0] * len(fns)
    for _ in range(reps):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            total[k] += time.perf_counter() - t0
    return [t * 1e3 / reps for t in total]


def tails_few_points(M, probs, reps):
    distrs, ok = mixtures(M, 25)
    t_ms, q_ms = alternating([lambda: sd.tail_means(distrs, probs), lambda: sd.quantiles(distrs, probs)], reps)
    q, lower, upper, _ = sd.tail_means(distrs, probs)
    sub_d, sub_k = distrs[:4], np.linspace(0, len(probs) - 1, 3).astype(int)
    t0 = time.perf_counter()
    worst = 0.0
    for d, qd, ud in zip(sub_d, q, upper):
        for k in sub_k:
            x = d.quantile(probs[k])[0]
            num = quad(lambda v: v * d.density(v)[0], x, DOM[1], epsabs=1e-12, epsrel=1e-12)[0]
            den = quad(lambda v: d.density(v)[0], x, DOM[1], epsabs=1e-12, epsrel=1e-12)[0]
            worst = max(worst, abs(num / den - ud[k]))
    sub_ms = (time.perf_counter() - t0) * 1e3
    quad_ms = sub_ms / (len(sub_d) * len(sub_k)) * M * len(probs)
    return dict(M=M, n_p=len(probs), tail_means_ms=round(t_ms, 3), quantiles_ms=round(q_ms, 3), quad_ms_scaled=round(quad_ms, 1),
                quad_subset=[len(sub_d), len(sub_k)], quad_vs_tail_means=float(worst), all_success=ok)


def tails_many_points(B, R1, n, reps):
    distrs, ok = mixtures(B, R1, seed=5)
    g = torch.Generator(device="cuda")
    g.manual_seed(B * 131 + R1)
    flat = torch.rand(B * n, dtype=torch.float64, device="cuda", generator=g)
    q, lower, upper = torch.empty_like(flat), torch.empty_like(flat), torch.empty_like(flat)
    torch.cuda.synchronize()
    handles, r1, lam, sig = sd._batch_problem_args(distrs)
    a, b = np.full(B, DOM[0]), np.full(B, DOM[1])
    cnt = np.full(B, n, dtype=np.int64)
    n_int, deg = distrs[0].n_intervals, distrs[0]._gauss_degree
    lib, P = _lib.lib(), _lib.ptr
    head = (B, C.cast(handles, C.c_void_p), P(r1), P(lam), P(sig), P(a), P(b), n_int, deg, P(flat), P(cnt))
    calls = [lambda: _lib.check(lib.mlmc_density_tail_means_batch(*head, P(q), P(lower), P(upper), None, None, _lib.DEVICE)),
             lambda: _lib.check(lib.mlmc_density_quantiles_batch(*head, P(q), None, _lib.DEVICE))]
    k_ms, k_n = C.c_double(), C.c_int64()
    for fn in calls:
        fn()
    wall, kern = [0.0, 0.0], [0.0, 0.0]
    for _ in range(reps):
        for k, fn in enumerate(calls):
            _lib.check(lib.mlmc_density_quantiles_kernel_time(C.byref(k_ms), C.byref(k_n)))       # reset
            t0 = time.perf_counter()
            fn()
            wall[k] += (time.perf_counter() - t0) * 1e3 / reps
            _lib.check(lib.mlmc_density_quantiles_kernel_time(C.byref(k_ms), C.byref(k_n)))
            kern[k] += k_ms.value / reps
    calls[0]()
    ordered = bool(torch.all((lower <= q) & (q <= upper)).item())
    return dict(B=B, R1=R1, n=n, tails_kernel_ms=round(kern[0], 3), quantile_kernel_ms=round(kern[1], 3), tails_call_ms=round(wall[0], 3),
                quantile_call_ms=round(wall[1], 3), ordered=ordered, all_success=ok)


def divergence_pairs(n_rep, n_comp, reps):
    distrs, ok = mixtures(n_comp + n_rep * n_comp, 25)
    priors = [distrs[m] for _ in range(n_rep) for m in range(n_comp)]
    posteriors = distrs[n_comp:]
    P = len(priors)
    d0 = distrs[0]
    pts, w = sd._composite_gauss(DOM, d0.n_intervals, d0._gauss_degree)
    first = np.tile(np.arange(n_comp), n_rep)

    def host_sums():
        rho = np.array(sd.densities(distrs, pts))
        rp, rq = rho[first], rho[n_comp:]
        d = np.log(rq) - np.log(rp)
        x = np.expm1(d)
        return ((rp * (x - d)) @ w, np.sqrt((rp * rp * x * x) @ w), 0.5 * (rp * np.abs(x)) @ w,
                np.sqrt(0.5 * (rp * np.expm1(0.5 * d) ** 2) @ w), rp @ w, rq @ w)
    big = P > 4000                                                   # the host alternative holds 5 arrays of P x 1344 doubles
    d_ms, h_ms = alternating([lambda: sd.divergences(priors, posteriors), host_sums], 1 if big else reps)
    res, host = sd.divergences(priors, posteriors), host_sums()
    rel = lambda got, want: float(np.max(np.abs(got - want) / np.abs(want)))
    sub = range(0, P, max(1, P // 4))[:4]
    t0 = time.perf_counter()
    worst = 0.0
    for k in sub:
        p, q = priors[k], posteriors[k]
        kl = sd.KL_divergence(lambda v: p.density(v)[0], lambda v: q.density(v)[0], DOM[0], DOM[1])
        l2 = sd.L2_distance(lambda v: p.density(v)[0], lambda v: q.density(v)[0], DOM[0], DOM[1])
        worst = max(worst, abs(kl - res.kl[k]) / res.kl[k], abs(l2 - res.l2[k]) / res.l2[k])
    quad_ms = (time.perf_counter() - t0) * 1e3 / len(sub) * P
    return dict(P=P, n_rep=n_rep, n_comp=n_comp, R1=25, rule=[d0.n_intervals, d0._gauss_degree], divergences_ms=round(d_ms, 3),
                host_sums_ms=round(h_ms, 3), quad_ms_scaled=round(quad_ms, 1), quad_pairs=len(sub),
                host_vs_entry=max(rel(host[0], res.kl), rel(host[1], res.l2)), quad_vs_entry=float(worst), all_success=ok)


def moments_batch(B, reps):
    distrs, ok = mixtures(B, 25)
    d0 = distrs[0]
    pts, w = sd._composite_gauss(DOM, d0.n_intervals, d0._gauss_degree)
    fn = d0.moments_fn

    def host_sums():
        rho = np.array(sd.densities(distrs, pts))
        phi = np.polynomial.legendre.legvander(fn.linear(pts), fn.size - 1)
        wr = rho * w
        mass = wr.sum(axis=1)
        return (wr @ phi) / mass[:, None], -(wr * np.log(rho)).sum(axis=1) / mass + np.log(mass), mass
    fns = [lambda: sd.density_moments(distrs), host_sums, lambda: sd.summaries(distrs)]
    for f in fns:
        f()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, f in enumerate(fns):
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    res, host = sd.density_moments(distrs), host_sums()
    span = lambda t: [round(min(t), 3), round(sum(t) / len(t), 3), round(max(t), 3)]
    return dict(B=B, R1=25, K=25, rule=[d0.n_intervals, d0._gauss_degree], moments_ms=span(times[0]), host_sums_ms=span(times[1]),
                summaries_ms=span(times[2]), host_vs_entry=float(np.max(np.abs(np.array(res.moments) - host[0]))),
                entropy_host_vs_entry=float(np.max(np.abs(res.entropy - host[1]))), all_success=ok)


def samples_shape(B, R1, n, reps):
    distrs, ok = mixtures(B, R1, seed=5)
    lib = _lib.lib()
    k_ms, k_n = C.c_double(), C.c_int64()
    seed = [1000 * B + R1]

    def new_route():
        seed[0] += 1                                                 # fresh draws in every call, as torch.rand gives the other route
        x = sd.samples(distrs, n, seed[0], device=True)
        torch.cuda.synchronize()
        return x

    def parent_route():
        u = torch.rand(B * n, dtype=torch.float64, device="cuda")
        x = sd.quantiles(distrs, list(torch.split(u, n)))
        torch.cuda.synchronize()
        return x
    routes = (new_route, parent_route)
    for fn in routes:
        fn()
    wall, kern = [[], []], [[], []]
    for _ in range(reps):
        for k, fn in enumerate(routes):
            _lib.check(lib.mlmc_density_quantiles_kernel_time(C.byref(k_ms), C.byref(k_n)))       # reset
            t0 = time.perf_counter()
            fn()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            _lib.check(lib.mlmc_density_quantiles_kernel_time(C.byref(k_ms), C.byref(k_n)))
            kern[k].append(k_ms.value)

    def ks(x):
        f = np.sort(sd.cdfs_on_rule([distrs[0]], x[0][:100_000].cpu().numpy())[0])
        k = np.arange(1, f.size + 1)
        return float(max(np.max(k / f.size - f), np.max(f - (k - 1) / f.size)))
    span = lambda t: [round(min(t), 3), round(sum(t) / len(t), 3), round(max(t), 3)]
    mean = lambda t: sum(t) / len(t)
    return dict(B=B, R1=R1, n=n, samples_ms=span(wall[0]), rand_quantiles_ms=span(wall[1]), samples_kernel_ms=span(kern[0]),
                quantiles_kernel_ms=span(kern[1]), speedup_wall=round(mean(wall[1]) / mean(wall[0]), 3),
                speedup_kernel=round(mean(kern[1]) / mean(kern[0]), 3), ks_samples=round(ks(new_route()), 5),
                ks_rand_quantiles=round(ks(parent_route()), 5), all_success=ok)


def joint_shape(M, R1, n, K, reps):
    """joint_samples(device=True) against (a) samples (independent draws) and (b) the route without the joint entry: torch.randn,
    torch.matmul with the factor, torch.special.ndtr, quantiles on the device uniforms; the routes take turns in one process"""
    distrs, ok = mixtures(M, R1, seed=5)
    lib = _lib.lib()
    k_ms, k_n = C.c_double(), C.c_int64()
    rng = np.random.default_rng(7)
    if K == M:
        A = rng.standard_normal((M, M + 3))
        c = A @ A.T
        d = 1.0 / np.sqrt(np.diag(c))
        factor = sd.correlation_factor(c * d[:, None] * d[None, :])[0]
    else:
        factor = rng.standard_normal((M, K))
        factor = np.ascontiguousarray(factor / np.sqrt(np.sum(factor * factor, axis=1))[:, None])
    factor_dev = torch.as_tensor(factor, device="cuda")
    seed = [1000 * M + R1]

    def joint_route():
        seed[0] += 1
        x = sd.joint_samples(distrs, n, seed[0], factor=factor, device=True)
        torch.cuda.synchronize()
        return x

    def independent_route():
        seed[0] += 1
        x = sd.samples(distrs, n, seed[0], device=True)
        torch.cuda.synchronize()
        return x

    def torch_route():
        z = torch.randn(K, n, dtype=torch.float64, device="cuda")
        u = torch.special.ndtr(torch.matmul(factor_dev, z)).clamp_(2.0 ** -53, 1.0 - 2.0 ** -53)
        x = sd.quantiles(distrs, list(u))
        torch.cuda.synchronize()
        return x
    routes = (joint_route, independent_route, torch_route)
    for fn in routes:
        fn()
    wall, kern = [[] for _ in routes], [[] for _ in routes]
    for _ in range(reps):
        for k, fn in enumerate(routes):
            _lib.check(lib.mlmc_density_quantiles_kernel_time(C.byref(k_ms), C.byref(k_n)))       # reset
            t0 = time.perf_counter()
            fn()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            _lib.check(lib.mlmc_density_quantiles_kernel_time(C.byref(k_ms), C.byref(k_n)))
            kern[k].append(k_ms.value)
    span = lambda t: [round(min(t), 3), round(sum(t) / len(t), 3), round(max(t), 3)]
    mean = lambda t: sum(t) / len(t)
    return dict(M=M, R1=R1, n=n, K=K, joint_ms=span(wall[0]), samples_ms=span(wall[1]), torch_quantiles_ms=span(wall[2]),
                joint_kernel_ms=span(kern[0]), samples_kernel_ms=span(kern[1]), quantiles_kernel_ms=span(kern[2]),
                joint_over_samples_wall=round(mean(wall[0]) / mean(wall[1]), 3), torch_over_joint_wall=round(mean(wall[2]) / mean(wall[0]), 3),
                all_success=ok)


def tcopula_shape(M, R1, n, K, dof, reps):
    """joint_samples(dof=...) against joint_samples of the same shape (the Gaussian entry), the two taking turns in one process
    after a warm-up each; and the elementwise entries on arrays of the call's sizes, which are the map and the mixing kernels on
    their own: student_t_cdf on M n values y = z s of the t law, chi2_mixing_scale on n uniforms"""
    distrs, ok = mixtures(M, R1, seed=5)
    lib = _lib.lib()
    k_ms, k_n = C.c_double(), C.c_int64()
    rng = np.random.default_rng(7)
    A = rng.standard_normal((M, M + 3))
    c = A @ A.T
    d = 1.0 / np.sqrt(np.diag(c))
    factor = sd.correlation_factor(c * d[:, None] * d[None, :])[0][:, :K] if K == M else None
    if factor is None:
        factor = rng.standard_normal((M, K))
        factor = np.ascontiguousarray(factor / np.sqrt(np.sum(factor * factor, axis=1))[:, None])
    seed = [1000 * M + R1]

    def t_route():
        seed[0] += 1
        x = sd.joint_samples(distrs, n, seed[0], factor=factor, device=True, dof=dof)
        torch.cuda.synchronize()
        return x

    def gauss_route():
        seed[0] += 1
        x = sd.joint_samples(distrs, n, seed[0], factor=factor, device=True)
        torch.cuda.synchronize()
        return x
    p0 = torch.rand(n, dtype=torch.float64, device="cuda").clamp_(2.0 ** -53, 1.0 - 2.0 ** -53)
    y = torch.randn(M, n, dtype=torch.float64, device="cuda") * sd.chi2_mixing_scale(p0, dof, device=True)[None, :]

    def map_route():
        u = sd.student_t_cdf(y, dof, device=True)
        torch.cuda.synchronize()
        return u

    def mixing_route():
        s = sd.chi2_mixing_scale(p0, dof, device=True)
        torch.cuda.synchronize()
        return s
    routes = (t_route, gauss_route, map_route, mixing_route)
    for fn in routes:
        fn()
    wall, kern = [[] for _ in routes], [[] for _ in routes]
    for _ in range(reps):
        for k, fn in enumerate(routes):
            _lib.check(lib.mlmc_density_quantiles_kernel_time(C.byref(k_ms), C.byref(k_n)))       # reset
            t0 = time.perf_counter()
            fn()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            _lib.check(lib.mlmc_density_quantiles_kernel_time(C.byref(k_ms), C.byref(k_n)))
            kern[k].append(k_ms.value)
    span = lambda t: [round(min(t), 3), round(sum(t) / len(t), 3), round(max(t), 3)]
    mean = lambda t: sum(t) / len(t)
    return dict(M=M, R1=R1, n=n, K=K, dof=dof, t_ms=span(wall[0]), gauss_ms=span(wall[1]), t_kernel_ms=span(kern[0]),
                gauss_kernel_ms=span(kern[1]), map_entry_ms=span(wall[2]), mixing_entry_ms=span(wall[3]),
                t_over_gauss_wall=round(mean(wall[0]) / mean(wall[1]), 3),
                t_over_gauss_kernel=round(mean(kern[0]) / mean(kern[1]), 3), all_success=ok)


def tconditional_shape(M, R1, B, n, dof, reps):
    """conditional_samples(dof=..., device=True) of B sets of n draws, component 0 of M given, against the Gaussian
    conditional_samples of the same shape, the two taking turns in one process after a warm-up each; and the elementwise entries on
    arrays of the call's sizes, which are the mixing kernel (n uniforms at dof + 1 degrees of freedom) and the map (B (M - 1) n
    values of the t law) on their own, as in tcopula_shape"""
    distrs, ok = mixtures(M, R1, seed=5)
    lib = _lib.lib()
    k_ms, k_n = C.c_double(), C.c_int64()
    rng = np.random.default_rng(7)
    A = rng.standard_normal((M, M + 3))
    c = A @ A.T
    d = 1.0 / np.sqrt(np.diag(c))
    corr = c * d[:, None] * d[None, :]
    cond_t, cond = sd.conditional_factor(corr, [0], return_observed=True), sd.conditional_factor(corr, [0])
    xs = sd.quantiles([distrs[0]], [np.linspace(0.05, 0.95, B) if B > 1 else np.array([0.3])])[0]
    seed = [1000 * M + R1]

    def t_route():
        seed[0] += 1
        x = sd.conditional_samples(distrs, n, seed[0], {0: xs}, factor_info=cond_t, device=True, dof=dof)
        torch.cuda.synchronize()
        return x

    def gauss_route():
        seed[0] += 1
        x = sd.conditional_samples(distrs, n, seed[0], {0: xs}, factor_info=cond, device=True)
        torch.cuda.synchronize()
        return x
    p0 = torch.rand(n, dtype=torch.float64, device="cuda").clamp_(2.0 ** -53, 1.0 - 2.0 ** -53)
    y = torch.randn(B * (M - 1), n, dtype=torch.float64, device="cuda") * sd.conditional_mixing_scale(p0, dof + 1.0, device=True)[None, :]

    def map_route():
        u = sd.student_t_cdf(y, dof, device=True)
        torch.cuda.synchronize()
        return u

    def mixing_route():
        sc = sd.conditional_mixing_scale(p0, dof + 1.0, device=True)
        torch.cuda.synchronize()
        return sc
    routes = (t_route, gauss_route, map_route, mixing_route)
    for fn in routes:
        fn()
    wall, kern = [[] for _ in routes], [[] for _ in routes]
    for _ in range(reps):
        for k, fn in enumerate(routes):
            _lib.check(lib.mlmc_density_quantiles_kernel_time(C.byref(k_ms), C.byref(k_n)))       # reset
            t0 = time.perf_counter()
            fn()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            _lib.check(lib.mlmc_density_quantiles_kernel_time(C.byref(k_ms), C.byref(k_n)))
            kern[k].append(k_ms.value)
    span = lambda t: [round(min(t), 3), round(sum(t) / len(t), 3), round(max(t), 3)]
    mean = lambda t: sum(t) / len(t)
    return dict(M=M, R1=R1, B=B, n=n, dof=dof, t_ms=span(wall[0]), gauss_ms=span(wall[1]), t_kernel_ms=span(kern[0]),
                gauss_kernel_ms=span(kern[1]), map_entry_ms=span(wall[2]), mixing_entry_ms=span(wall[3]),
                t_over_gauss_wall=round(mean(wall[0]) / mean(wall[1]), 3),
                t_over_gauss_kernel=round(mean(kern[0]) / mean(kern[1]), 3), all_success=ok)


def conditional_shape(M, R1, B, n, reps):
    """conditional_samples(device=True) of B sets of n draws, component 0 of M given, against (a) a Python loop of B single-set calls
    and (b) joint_samples of the M - 1 other components with B n draws; the routes take turns in one process"""
    distrs, ok = mixtures(M, R1, seed=5)
    lib = _lib.lib()
    k_ms, k_n = C.c_double(), C.c_int64()
    rng = np.random.default_rng(7)
    A = rng.standard_normal((M, M + 3))
    c = A @ A.T
    d = 1.0 / np.sqrt(np.diag(c))
    cond = sd.conditional_factor(c * d[:, None] * d[None, :], [0])
    unit = np.ascontiguousarray(cond[1] / cond[2].s[:, None])                  # rows of unit norm: what joint_samples takes
    xs = sd.quantiles([distrs[0]], [np.linspace(0.05, 0.95, B) if B > 1 else np.array([0.3])])[0]
    seed = [1000 * M + R1]

    def batched_route():
        seed[0] += 1
        x = sd.conditional_samples(distrs, n, seed[0], {0: xs}, factor_info=cond, device=True)
        torch.cuda.synchronize()
        return x

    def loop_route():
        seed[0] += 1
        x = [sd.conditional_samples(distrs, n, seed[0], {0: float(v)}, factor_info=cond, device=True) for v in xs]
        torch.cuda.synchronize()
        return x

    def joint_route():
        seed[0] += 1
        x = sd.joint_samples(distrs[1:], B * n, seed[0], factor=unit, device=True)
        torch.cuda.synchronize()
        return x
    routes = (batched_route, loop_route, joint_route)
    for fn in routes:
        fn()
    wall, kern = [[] for _ in routes], [[] for _ in routes]
    for _ in range(reps):
        for k, fn in enumerate(routes):
            _lib.check(lib.mlmc_density_quantiles_kernel_time(C.byref(k_ms), C.byref(k_n)))       # reset
            t0 = time.perf_counter()
            fn()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            _lib.check(lib.mlmc_density_quantiles_kernel_time(C.byref(k_ms), C.byref(k_n)))
            kern[k].append(k_ms.value)
    span = lambda t: [round(min(t), 3), round(float(np.median(t)), 3), round(max(t), 3)]
    med = lambda t: float(np.median(t))
    return dict(M=M, R1=R1, B=B, n=n, conditional_ms=span(wall[0]), loop_ms=span(wall[1]), joint_ms=span(wall[2]),
                conditional_kernel_ms=span(kern[0]), loop_kernel_ms=span(kern[1]), joint_kernel_ms=span(kern[2]),
                loop_over_conditional_wall=round(med(wall[1]) / med(wall[0]), 3),
                conditional_over_joint_wall=round(med(wall[0]) / med(wall[2]), 3), all_success=ok)


def qmc_pair(call, reps):
    """wall and kernel ms of call(qmc=False) and call(qmc=True), the two taking turns inside every repetition on the same box"""
    lib = _lib.lib()
    k_ms, k_n = C.c_double(), C.c_int64()
    for flag in (False, True):
        call(flag)
    wall, kern = [[], []], [[], []]
    for _ in range(reps):
        for k, flag in enumerate((False, True)):
            _lib.check(lib.mlmc_density_quantiles_kernel_time(C.byref(k_ms), C.byref(k_n)))       # reset
            t0 = time.perf_counter()
            call(flag)
            wall[k].append((time.perf_counter() - t0) * 1e3)
            _lib.check(lib.mlmc_density_quantiles_kernel_time(C.byref(k_ms), C.byref(k_n)))
            kern[k].append(k_ms.value)
    span = lambda t: [round(min(t), 3), round(float(np.median(t)), 3), round(max(t), 3)]
    med = lambda t: float(np.median(t))
    return dict(philox_ms=span(wall[0]), qmc_ms=span(wall[1]), philox_kernel_ms=span(kern[0]), qmc_kernel_ms=span(kern[1]),
                qmc_over_philox_wall=round(med(wall[1]) / med(wall[0]), 3), qmc_over_philox_kernel=round(med(kern[1]) / med(kern[0]), 3))


def qmc_times(reps, quick):
    """samples, joint_samples and conditional_samples with and without qmc on the shapes of --samples, --joint and --conditional"""
    out = dict(samples=[], joint=[], conditional=[])
    seed = [77]

    def fresh():
        seed[0] += 1
        return seed[0]
    for B, R1, n in ([(4, 9, 10_000)] if quick else [(1, 9, 10_000_000), (1, 25, 10_000_000), (1, 64, 10_000_000), (64, 25, 1_000_000),
                                                    (3600, 25, 1_000)]):
        distrs, ok = mixtures(B, R1, seed=5)
        streams = np.arange(B) % 1024                        # dimensions under qmc; the same streams for both variants

        def call(qmc):
            x = sd.samples(distrs, n, fresh(), streams=streams, device=True, qmc=qmc)
            torch.cuda.synchronize()
            return x
        out["samples"].append(dict(B=B, R1=R1, n=n, all_success=ok, **qmc_pair(call, reps)))
        print(json.dumps(out["samples"][-1]), file=sys.stderr, flush=True)                 # progress; the result line goes to stdout
    rng = np.random.default_rng(7)
    for M, R1, n, K in ([(4, 9, 10_000, 4)] if quick else [(12, 25, 1_000_000, 12), (64, 25, 1_000_000, 64), (256, 25, 100_000, 256),
                                                          (12, 25, 1_000_000, 3)]):
        distrs, ok = mixtures(M, R1, seed=5)
        factor = rng.standard_normal((M, K))
        factor = np.ascontiguousarray(factor / np.sqrt(np.sum(factor * factor, axis=1))[:, None])

        def call(qmc):
            x = sd.joint_samples(distrs, n, fresh(), factor=factor, device=True, qmc=qmc)
            torch.cuda.synchronize()
            return x
        out["joint"].append(dict(M=M, R1=R1, n=n, K=K, all_success=ok, **qmc_pair(call, reps)))
        print(json.dumps(out["joint"][-1]), file=sys.stderr, flush=True)                 # progress; the result line goes to stdout
    for M, R1, B, n in ([(4, 9, 3, 1_000)] if quick else [(12, 25, 1, 1_000_000), (12, 25, 64, 10_000), (12, 25, 1024, 1_000)]):
        distrs, ok = mixtures(M, R1, seed=5)
        A = rng.standard_normal((M, M + 3))
        c = A @ A.T
        d = 1.0 / np.sqrt(np.diag(c))
        cond = sd.conditional_factor(c * d[:, None] * d[None, :], [0])
        xs = sd.quantiles([distrs[0]], [np.linspace(0.05, 0.95, B) if B > 1 else np.array([0.3])])[0]

        def call(qmc):
            x = sd.conditional_samples(distrs, n, fresh(), {0: xs}, factor_info=cond, device=True, qmc=qmc)
            torch.cuda.synchronize()
            return x
        out["conditional"].append(dict(M=M, R1=R1, B=B, n=n, all_success=ok, **qmc_pair(call, reps)))
        print(json.dumps(out["conditional"][-1]), file=sys.stderr, flush=True)                 # progress; the result line goes to stdout
    return out


CORR3 = np.array([[1.0, 0.8, -0.5], [0.8, 1.0, -0.2], [-0.5, -0.2, 1.0]])


def qmc_errors(quick):
    """RMS error over seeds 1 .. 8 of the mean of g(u) from joint_samples, with and without qmc, n = 2^10, 2^12, .. 2^20:
    g = prod_m (1 + 0.8 (u_m - 1/2)) under M = K = 4, F = I (exact 1), and g = u_0 u_1 under CORR3 (exact 1/4 + arcsin(rho / 2) / 2 pi)"""
    distrs, _ = mixtures(4, 9, seed=5)
    cases = (("product4", distrs, np.eye(4), lambda u: torch.prod(1.0 + 0.8 * (u - 0.5), dim=0), 1.0),
             ("u0u1_corr3", distrs[:3], sd.correlation_factor(CORR3)[0], lambda u: u[0] * u[1],
              0.25 + float(np.arcsin(CORR3[0, 1] / 2.0)) / (2.0 * np.pi)))
    rows = []
    for tag, ds, factor, g, exact in cases:
        for k in ((10, 12) if quick else range(10, 21, 2)):
            rms = []
            for qmc in (False, True):
                err = [float(g(sd.joint_samples(ds, 2 ** k, seed, factor=factor, device=True, return_uniforms=True, qmc=qmc)[1]).mean())
                       - exact for seed in range(1, 9)]
                rms.append(float(np.sqrt(np.mean(np.square(err)))))
            rows.append(dict(integrand=tag, n=2 ** k, philox_rms=float("%.3g" % rms[0]), qmc_rms=float("%.3g" % rms[1]),
                             philox_over_qmc=round(rms[0] / rms[1], 1)))
    return rows


def equicorrelated_exceedance(M, t, rho=0.5):
    """P(Y_m > t for all m) for M equicorrelated standard normals: with a common factor x, Y_m = sqrt(rho) x + sqrt(1 - rho) e_m, the
    integral over x of phi(x) Phi((sqrt(rho) x - t) / sqrt(1 - rho))^M, by adaptive quadrature"""
    from scipy.special import log_ndtr
    g = lambda x: np.exp(-0.5 * x * x + M * log_ndtr((np.sqrt(rho) * x - t) / np.sqrt(1.0 - rho))) / np.sqrt(2.0 * np.pi)
    return quad(g, -12.0, 12.0, epsabs=0.0, epsrel=1e-12, limit=400)[0]


def boxprob_shape(M, B, n, reps, t, seeds=tuple(range(1, 9))):
    """copula_box_probabilities of B copies of the box (t, inf)^M under equicorrelation 1/2 (t = 0: the orthant, exactly
    1 / (M + 1); otherwise the one-dimensional integral above), R = 8 seeds in one call: the time per call and the RMS over the seeds
    of the relative error of a seed's mean, next to the counting route at the same n on the same box: joint_samples on the
    device (one call per seed), the comparison of the copula uniforms with Phi(t) and the mean in torch."""
    from scipy.special import ndtr
    corr = np.full((M, M), 0.5)
    np.fill_diagonal(corr, 1.0)
    low = np.linalg.cholesky(corr)
    exact = 1.0 / (M + 1) if t == 0.0 else equicorrelated_exceedance(M, t)
    lo, hi = np.full((B, M), t), np.full((B, M), np.inf)
    ms, res = timed(lambda: sd.copula_box_probabilities(low, lo, hi, n, seeds), reps)
    rms = float(np.sqrt(np.mean(np.square(res.replicates[:, 0] / exact - 1.0))))
    distrs, _ = mixtures(M, 9, seed=5)
    factor = low / np.sqrt(np.sum(low * low, axis=1))[:, None]
    level = float(ndtr(t))

    def count(seed):
        u = sd.joint_samples(distrs, n, seed, factor=factor, device=True, return_uniforms=True)[1]
        return float(torch.all(u > level, dim=0).double().mean())
    count_ms, _ = timed(lambda: count(seeds[0]), reps)
    counted = np.array([count(s) for s in seeds])
    return dict(M=M, B=B, n=n, R=len(seeds), threshold=round(t, 4), exact=float("%.6g" % exact), prob=float("%.6g" % res.prob[0]),
                stderr=float("%.3g" % res.stderr[0]), call_ms=round(ms, 3), ms_per_box_and_seed=round(ms / (B * len(seeds)), 4),
                rel_rms=float("%.3g" % rms), count_ms_per_seed=round(count_ms, 3),
                count_rel_rms=float("%.3g" % np.sqrt(np.mean(np.square(counted / exact - 1.0)))),
                count_zero_seeds=int(np.sum(counted == 0.0)))


def boxdraws_shape(M, n, reps, p, seeds=tuple(range(1, 9))):
    """event_samples(device=True) of the event "components 0 and 1 exceed their p-quantile" for M mixture marginals under
    equicorrelation 1/2, R = 8 seeds in one call, next to rejection: joint_samples(device=True) of the same n per seed and a filter
    in torch.  For both routes the scenarios inside the event per millisecond (all R n of the call; what the filter keeps) and the
    standard error over the seeds of the conditional mean of component 2 (of component 0 for M = 2)."""
    corr = np.full((M, M), 0.5)
    np.fill_diagonal(corr, 1.0)
    distrs, _ = mixtures(M, 9, seed=5)
    factor = sd.correlation_factor(corr)[0]
    t = np.array([sd.quantiles([distrs[m]], [np.array([p])])[0][0] for m in (0, 1)])
    lower = np.full(M, -np.inf)
    lower[:2] = t
    comp = 2 if M > 2 else 0
    R = len(seeds)

    def event():
        ev = sd.event_samples(distrs, lower, np.inf, n, seeds, factor=factor, device=True)
        torch.cuda.synchronize()
        return ev
    ms, ev = timed(event, reps)
    f, x = ev.weights[:, 0], ev.draws[:, 0, comp]
    ratio = ((f * x).sum(dim=1) / f.sum(dim=1)).cpu().numpy()
    prob, ess = float(ev.prob.prob[0]), float(np.mean(ev.ess)) / n
    del ev, f, x

    def reject(seed):
        x = sd.joint_samples(distrs, n, seed, factor=factor, device=True)
        inside = (x[0] > t[0]) & (x[1] > t[1])
        kept = int(inside.sum())
        return kept, float(x[comp][inside].mean()) if kept else float("nan")
    rej_ms, _ = timed(lambda: reject(seeds[0]), reps)
    rejected = [reject(s) for s in seeds]
    kept = np.array([k for k, _ in rejected], dtype=np.float64)
    means = np.array([m for _, m in rejected])
    return dict(M=M, n=n, R=R, quantile=p, prob=float("%.6g" % prob),
                call_ms=round(ms, 3), inside_per_ms=float("%.4g" % (R * n / ms)), ess_fraction=float("%.3g" % ess),
                event_mean=float("%.8g" % ratio.mean()), event_stderr=float("%.3g" % (np.std(ratio, ddof=1) / np.sqrt(R))),
                reject_ms_per_seed=round(rej_ms, 3), reject_inside_per_ms=float("%.4g" % (kept.mean() / rej_ms)),
                reject_mean=float("%.8g" % np.nanmean(means)) if np.any(kept > 0) else None,
                reject_stderr=float("%.3g" % (np.nanstd(means, ddof=1) / np.sqrt(np.sum(kept > 0)))) if np.sum(kept > 0) > 1 else None,
                reject_zero_seeds=int(np.sum(kept == 0)))


def _turns(routes, reps):
    """[min, mean, max] wall ms of every route, the routes taking turns after a warm-up call each"""
    for fn in routes:
        fn()
    wall = [[] for _ in routes]
    for _ in range(reps):
        for k, fn in enumerate(routes):
            t0 = time.perf_counter()
            fn()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    return [[round(min(t), 3), round(sum(t) / len(t), 3), round(max(t), 3)] for t in wall]


def _t_parts(dof, n_mix, n_map):
    """the mixing kernel and the CDF pass of a t box call on their own: chi2_mixing_scale on n_mix device uniforms and student_t_cdf
    on n_map device values of the t law, each with its entry's launch and wait"""
    p0 = torch.rand(n_mix, dtype=torch.float64, device="cuda").clamp_(2.0 ** -53, 1.0 - 2.0 ** -53)
    y = None
    if n_map:
        y = torch.randn(n_map, dtype=torch.float64, device="cuda") * sd.chi2_mixing_scale(p0, dof, device=True)[torch.arange(n_map, device="cuda") % n_mix]

    def mixing_route():
        sd.chi2_mixing_scale(p0, dof, device=True)
        torch.cuda.synchronize()

    def map_route():
        sd.student_t_cdf(y, dof, device=True)
        torch.cuda.synchronize()
    return (mixing_route, map_route) if n_map else (mixing_route,)


def tboxprob_shape(M, B, n, reps, t, dof, seeds=tuple(range(1, 9))):
    """copula_box_probabilities(dof=...) of B copies of the box (t, inf)^M in t-score space under equicorrelation 1/2 against the
    Gaussian call of the same shape (the same numbers as limits: the work is the same, the probabilities are not), the two taking
    turns in one process; and the mixing kernel on its own, chi2_mixing_scale on the call's R n uniforms"""
    corr = np.full((M, M), 0.5)
    np.fill_diagonal(corr, 1.0)
    low = np.linalg.cholesky(corr)
    lo, hi = np.full((B, M), t), np.full((B, M), np.inf)
    got = {}

    def t_route():
        got["t"] = sd.copula_box_probabilities(low, lo, hi, n, seeds, dof=dof)

    def gauss_route():
        got["g"] = sd.copula_box_probabilities(low, lo, hi, n, seeds)
    wall = _turns((t_route, gauss_route) + _t_parts(dof, len(seeds) * n, 0), reps)
    return dict(M=M, B=B, n=n, R=len(seeds), threshold=round(t, 4), dof=dof, t_ms=wall[0], gauss_ms=wall[1], mixing_entry_ms=wall[2],
                t_over_gauss_wall=round(wall[0][1] / wall[1][1], 3), prob=float("%.6g" % got["t"].prob[0]),
                stderr=float("%.3g" % got["t"].stderr[0]), gauss_prob=float("%.6g" % got["g"].prob[0]),
                gauss_stderr=float("%.3g" % got["g"].stderr[0]))


def tlead_shape(M, B, n, reps, t, dof, seeds=tuple(range(1, 9))):
    """copula_box_probabilities(dof=..., mixing="conditioned") of B copies of the box (t, inf)^M in t-score space under equicorrelation
    1/2 against the plain t call of the same shape, the two taking turns in one process; ess / n of either from the integrand of one
    box in a call of its own"""
    corr = np.full((M, M), 0.5)
    np.fill_diagonal(corr, 1.0)
    low = np.linalg.cholesky(corr)
    lo, hi = np.full((B, M), t), np.full((B, M), np.inf)
    got = {}

    def lead_route():
        got["l"] = sd.copula_box_probabilities(low, lo, hi, n, seeds, dof=dof, mixing="conditioned")

    def plain_route():
        got["p"] = sd.copula_box_probabilities(low, lo, hi, n, seeds, dof=dof)
    wall = _turns((lead_route, plain_route), reps)

    def ess(**kw):
        f = sd.copula_box_probabilities(low, lo[0], hi[0], n, seeds, dof=dof, return_integrand=True, **kw)[1][:, 0]
        with np.errstate(invalid="ignore", divide="ignore"):
            return float("%.4g" % np.nanmean(f.sum(axis=1) ** 2 / (n * (f * f).sum(axis=1))))
    return dict(M=M, B=B, n=n, R=len(seeds), threshold=round(t, 4), dof=dof, lead_ms=wall[0], plain_ms=wall[1],
                lead_over_plain_wall=round(wall[0][1] / wall[1][1], 3), prob=float("%.6g" % got["l"].prob[0]),
                stderr=float("%.3g" % got["l"].stderr[0]), ess_fraction=ess(mixing="conditioned"),
                plain_prob=float("%.6g" % got["p"].prob[0]), plain_stderr=float("%.3g" % got["p"].stderr[0]), plain_ess_fraction=ess())


def _ascending_problem(M, B):
    """B boxes under equicorrelation 1/2 whose lower limits rise from -2 to 2.5 over the components (no upper limits), each box
    rotated by its index so that the boxes differ: the case `asc` of DESIGN.md 3.5.28 at any M"""
    corr = np.full((M, M), 0.5)
    np.fill_diagonal(corr, 1.0)
    lo = np.stack([np.roll(np.linspace(-2.0, 2.5, M), b) for b in range(B)])
    return corr, lo, np.full((B, M), np.inf)


def boxorder_kernel_shape(M, B, reps):
    """box_order alone (upload, the order kernel, download, one wait) for B boxes of M components, one shared covariance"""
    corr, lo, hi = _ascending_problem(M, B)
    wall = _turns((lambda: sd.box_order(corr, lo, hi),), reps)
    return dict(M=M, B=B, order_ms=wall[0])


def boxorder_call_shape(M, B, n, reps, seeds=tuple(range(1, 9))):
    """the reordered chain call (box_order, then copula_box_probabilities with one factor per box) against the natural call of the
    same shape (one shared factor), the two taking turns in one process, with the probability and standard error of box 0"""
    corr, lo, hi = _ascending_problem(M, B)
    low = np.linalg.cholesky(corr)
    got = {}

    def ordered_route():
        o = sd.box_order(corr, lo, hi)
        got["o"] = sd.copula_box_probabilities(o.factor, o.lower, o.upper, n, seeds)

    def natural_route():
        got["n"] = sd.copula_box_probabilities(low, lo, hi, n, seeds)
    wall = _turns((ordered_route, natural_route), reps)
    return dict(M=M, B=B, n=n, R=len(seeds), ordered_ms=wall[0], natural_ms=wall[1],
                ordered_over_natural_wall=round(wall[0][1] / wall[1][1], 3), prob=float("%.6g" % got["o"].prob[0]),
                stderr=float("%.3g" % got["o"].stderr[0]), natural_prob=float("%.6g" % got["n"].prob[0]),
                natural_stderr=float("%.3g" % got["n"].stderr[0]))


def boxorder_bands_shape(M, B, n, reps, seeds=tuple(range(1, 9))):
    """the bands of a joint exceedance over B replicate correlation matrices: ONE call with one factor per box
    (joint_probabilities_over_correlations) against the loop of B + 1 joint_probabilities calls that it replaces, the two taking
    turns in one process; the replicates are perturbed equicorrelation matrices, the marginals uniform"""
    from scipy.special import ndtr
    from tests import score_cases as sk
    distrs = [sk.closed_distribution(0.0, (0.0, 1.0)) for _ in range(M)]
    rng = np.random.default_rng(17)
    corrs = []
    for _ in range(B + 1):
        a = np.linalg.cholesky(_ascending_problem(M, 1)[0]) @ rng.standard_normal((M, 40 * M))
        c = np.corrcoef(a)
        corrs.append(0.5 * (c + c.T))
    corrs = np.array(corrs)
    x = ndtr(np.linspace(-1.0, 1.5, M))
    got = {}

    def one_call():
        got["one"] = sd.joint_probabilities_over_correlations(distrs, x, np.inf, n, seeds, corrs)[0]

    def loop():
        got["loop"] = [sd.joint_probabilities(distrs, x, np.inf, n, seeds, corr=c) for c in corrs]
    wall = _turns((one_call, loop), reps)
    same = all(np.array_equal(a.replicates, b.replicates) for a, b in zip(got["one"], got["loop"]))
    return dict(M=M, replicates=B, n=n, R=len(seeds), one_call_ms=wall[0], loop_ms=wall[1],
                loop_over_one_call_wall=round(wall[1][1] / wall[0][1], 2), bit_identical=bool(same))


def _tcond_problem(M, B, t):
    """B boxes (t, inf)^M in t-score space under equicorrelation 1/2, each with the conditional location and scale of its own given
    t score of one further component: y_O in (0, 3], mu = y_O / 2, r^2 = (nu + y_O^2) / (nu + 1) with nu filled in by the caller"""
    corr = np.full((M + 1, M + 1), 0.5)
    np.fill_diagonal(corr, 1.0)
    _, fc, _, _ = sd.conditional_factor(corr, [0], return_observed=True)
    y_obs = 3.0 * np.arange(1, B + 1) / B
    return fc, np.full((B, M), t), np.full((B, M), np.inf), np.repeat(0.5 * y_obs[:, None], M, axis=1), y_obs


def tcondbox_shape(M, B, n, reps, t, dof, draws=False, seeds=tuple(range(1, 9))):
    """conditional_box_probabilities (draws: conditional_box_draws with device outputs) of B sets of given values, p = 1, against the t
    entry of the same factor, limits and shape, the two taking turns in one process"""
    fc, lo, hi, shift, y_obs = _tcond_problem(M, B, t)
    scale = np.sqrt((dof + y_obs * y_obs) / (dof + 1.0))
    got = {}

    def cond_route():
        if draws:
            got["c"] = sd.conditional_box_draws(fc, lo, hi, n, seeds, dof, dof_mix=dof + 1.0, shift=shift, scale=scale, device=True).prob
            torch.cuda.synchronize()
        else:
            got["c"] = sd.conditional_box_probabilities(fc, lo, hi, n, seeds, dof, dof_mix=dof + 1.0, shift=shift, scale=scale)

    def t_route():
        if draws:
            got["t"] = sd.copula_box_draws(fc, lo, hi, n, seeds, dof=dof, device=True).prob
            torch.cuda.synchronize()
        else:
            got["t"] = sd.copula_box_probabilities(fc, lo, hi, n, seeds, dof=dof)
    p0 = torch.rand(len(seeds) * n, dtype=torch.float64, device="cuda").clamp_(2.0 ** -53, 1.0 - 2.0 ** -53)

    def cond_mixing_route():
        sd.conditional_mixing_scale(p0, dof + 1.0, device=True)
        torch.cuda.synchronize()

    def t_mixing_route():
        sd.chi2_mixing_scale(p0, dof, device=True)
        torch.cuda.synchronize()
    wall = _turns((cond_route, t_route, cond_mixing_route, t_mixing_route), reps)
    return dict(M=M, B=B, n=n, R=len(seeds), threshold=round(t, 4), dof=dof, dof_mix=dof + 1.0, draws=draws, cond_ms=wall[0], t_ms=wall[1],
                cond_mixing_entry_ms=wall[2], t_mixing_entry_ms=wall[3],
                cond_over_t_wall=round(wall[0][1] / wall[1][1], 3), prob=float("%.6g" % got["c"].prob[0]),
                stderr=float("%.3g" % got["c"].stderr[0]), t_prob=float("%.6g" % got["t"].prob[0]),
                t_stderr=float("%.3g" % got["t"].stderr[0]))


def tboxdraws_shape(M, n, reps, p, dof, seeds=tuple(range(1, 9))):
    """event_samples(dof=..., device=True) of the event of --boxdraws against the Gaussian call of the same shape, the two taking
    turns in one process; and the mixing kernel and the CDF pass on their own, on R n uniforms and R M n scores"""
    corr = np.full((M, M), 0.5)
    np.fill_diagonal(corr, 1.0)
    distrs, _ = mixtures(M, 9, seed=5)
    factor = sd.correlation_factor(corr)[0]
    lower = np.full(M, -np.inf)
    lower[:2] = [sd.quantiles([distrs[m]], [np.array([p])])[0][0] for m in (0, 1)]
    got = {}

    def route(key, dof):
        def run():
            ev = sd.event_samples(distrs, lower, np.inf, n, seeds, factor=factor, device=True, dof=dof)
            torch.cuda.synchronize()
            got[key] = (float(ev.prob.prob[0]), float(np.mean(ev.ess)) / n)
        return run
    R = len(seeds)
    wall = _turns((route("t", dof), route("g", None)) + _t_parts(dof, R * n, R * M * n), reps)
    return dict(M=M, n=n, R=R, quantile=p, dof=dof, t_ms=wall[0], gauss_ms=wall[1], mixing_entry_ms=wall[2], map_entry_ms=wall[3],
                t_over_gauss_wall=round(wall[0][1] / wall[1][1], 3), prob=float("%.6g" % got["t"][0]),
                ess_fraction=float("%.3g" % got["t"][1]), gauss_prob=float("%.6g" % got["g"][0]),
                gauss_ess_fraction=float("%.3g" % got["g"][1]))


def scores_shape(M, R1, n, reps, levels=0):
    """normal_scores(device=True) of n (fine, coarse) pairs of M components against the route without the entry: cdfs_on_rule on the
    device tensors of fine and of coarse, then torch clamp and torch.special.ndtri (which has no drop of out-of-domain values: the
    inputs here are all in-domain); the two routes take turns in one process.  levels > 0: in addition
    Estimate.estimate_score_correlation against estimate_component_covariance on a DeviceMemory store of that many levels of n
    pairs each, end to end."""
    distrs, ok = mixtures(M, R1, seed=5)
    lib = _lib.lib()
    k_ms, k_n = C.c_double(), C.c_int64()
    gen = torch.Generator(device="cuda").manual_seed(1000 * M + R1)
    fine = (torch.rand(M, n, dtype=torch.float64, device="cuda", generator=gen) * 0.96 + 0.02) * (DOM[1] - DOM[0]) + DOM[0]
    coarse = (fine + 0.05 * torch.randn(M, n, dtype=torch.float64, device="cuda", generator=gen)).clamp_(DOM[0] + 0.1, DOM[1] - 0.1)

    def scores_route():
        z = sd.normal_scores(distrs, fine, coarse, device=True)
        torch.cuda.synchronize()
        return z

    def cdf_route():
        z = [torch.special.ndtri(torch.stack(sd.cdfs_on_rule(distrs, list(x))).clamp_(2.0 ** -53, 1.0 - 2.0 ** -53)) for x in (fine, coarse)]
        torch.cuda.synchronize()
        return z
    routes = (scores_route, cdf_route)
    results = [fn() for fn in routes]
    # the two routes share Fhat bit for bit; normcdfinv and torch's ndtri agree to rounding
    diff = max(float((a - b).abs().max()) for a, b in zip(*results))
    del results
    wall, kern = [[] for _ in routes], [[] for _ in routes]
    for _ in range(reps):
        for k, fn in enumerate(routes):
            _lib.check(lib.mlmc_density_quantiles_kernel_time(C.byref(k_ms), C.byref(k_n)))       # reset
            t0 = time.perf_counter()
            fn()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            _lib.check(lib.mlmc_density_quantiles_kernel_time(C.byref(k_ms), C.byref(k_n)))
            kern[k].append(k_ms.value)
    span = lambda t: [round(min(t), 3), round(sum(t) / len(t), 3), round(max(t), 3)]
    mean = lambda t: sum(t) / len(t)
    # one partial-cell rule per value: 21 nodes x (2 R1 + EXP_FLOPS) operations, as many_points counts them
    deg = distrs[0]._gauss_degree
    flops = 2.0 * M * n * deg * (2 * R1 + EXP_FLOPS)
    out = dict(M=M, R1=R1, n=n, scores_ms=span(wall[0]), cdf_ndtri_ms=span(wall[1]), scores_kernel_ms=span(kern[0]),
               cdf_kernel_ms=span(kern[1]), cdf_over_scores_wall=round(mean(wall[1]) / mean(wall[0]), 3),
               scores_kernel_share_of_fp64_peak=round(flops / (mean(kern[0]) * 1e-3) / PEAK_FP64, 4), max_abs_diff_z=diff, all_success=ok)
    if levels > 0:
        from mlmc_amd.estimator import Estimate
        from mlmc_amd.quantity import quantity_estimate as qe
        from mlmc_amd.quantity.quantity import make_root_quantity
        from mlmc_amd.quantity.quantity_spec import QuantitySpec
        from mlmc_amd.sample_storage import DeviceMemory
        spec = [QuantitySpec(name="q", unit="m", shape=(M, 1), times=[1], locations=['0'])]
        dev = DeviceMemory()
        dev.save_global_data(result_format=spec, level_parameters=[[0.5 ** l] for l in range(levels)])
        for l in range(levels):
            dev.set_level_samples(l, torch.stack([fine, coarse if l > 0 else torch.zeros_like(fine)], dim=-1))
        qe.device_cache_clear()
        est = Estimate(make_root_quantity(dev, spec)['q'], dev, Legendre(R1, DOM))
        pdfs = [(d, None, None, None) for d in distrs]
        est_ms = alternating([lambda: est.estimate_score_correlation(densities=pdfs), lambda: est.estimate_component_covariance()], reps)
        out.update(levels=levels, score_correlation_ms=round(est_ms[0], 3), component_covariance_ms=round(est_ms[1], 3))
    return out


STREAM_RATE = 5.4e12     # bytes / s of this package's own streaming kernels


def aggregates_shape(S, M, n, reps):
    """mlmc_scenario_aggregates on S sets of M x n device-resident scenarios, A = 3 linear rows, all extremes and the count (Q = 8),
    against the torch composition on the same materialised matrix, the two taking turns"""
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    x = torch.randn((S, M, n), dtype=torch.float64, device=dev, generator=gen)
    rng = np.random.default_rng(6)
    W = np.ascontiguousarray(rng.uniform(-1.0, 1.0, (3, M)))
    lower, upper = np.full(M, -1.0), np.full(M, 1.5)
    extras = _lib.AGG_MAX | _lib.AGG_MIN | _lib.AGG_COUNT | _lib.AGG_ARGMAX | _lib.AGG_ARGMIN
    Q = 3 + 5
    out = torch.empty((S, Q, n), dtype=torch.float64, device=dev)
    Wd, lo_d, hi_d = torch.from_numpy(W).to(dev), torch.from_numpy(lower).to(dev)[:, None], torch.from_numpy(upper).to(dev)[:, None]
    torch.cuda.synchronize()
    lib = _lib.lib()

    def entry():
        _lib.check(lib.mlmc_scenario_aggregates(_lib.ptr(x), S, M, n, n, _lib.ptr(W), 3, None, _lib.ptr(lower), _lib.ptr(upper), extras,
                                                _lib.ptr(out), n, _lib.DEVICE))

    def composition():
        lin = torch.matmul(Wd, x)
        mx, amx = torch.max(x, dim=-2)
        mn, amn = torch.min(x, dim=-2)
        cnt = ((x <= lo_d) | (x >= hi_d)).sum(dim=-2)
        torch.cuda.synchronize()
        return lin, mx, mn, cnt, amx, amn

    entry_ms, torch_ms = alternating([entry, composition], reps)
    # the kernel's own time: HIP events on the stream the library launches on (main binds it to torch's), around the call: three small
    # uploads and one launch
    entry()
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        entry()
        b.record()
        torch.cuda.synchronize()
        ev.append(a.elapsed_time(b))
    event_ms = float(np.median(ev))
    lin, mx, mn, cnt, amx, amn = composition()
    same_extras = bool(torch.equal(out[:, 3], mx) and torch.equal(out[:, 4], mn) and torch.equal(out[:, 5], cnt.to(torch.float64))
                       and torch.equal(out[:, 6], amx.to(torch.float64)) and torch.equal(out[:, 7], amn.to(torch.float64)))
    lin_err = float((out[:, :3] - lin).abs().max() / lin.abs().max())
    alg_bytes = 8.0 * S * n * (M + Q)
    rate = alg_bytes / (event_ms * 1e-3)
    return dict(S=S, M=M, n=n, A=3, Q=Q, entry_ms=round(entry_ms, 3), torch_ms=round(torch_ms, 3), torch_over_entry_wall=round(torch_ms / entry_ms, 2),
                event_ms=round(event_ms, 4), alg_gbytes=round(alg_bytes / 1e9, 4), tbytes_per_s=round(rate / 1e12, 3),
                fraction_of_stream_rate=round(rate / STREAM_RATE, 3), extras_equal_torch=same_extras, linear_rel_diff_torch=lin_err)


HBM_PEAK = 8.0e12        # bytes / s, MI355X data sheet


def concordance_shape(M, n, reps, G=3):
    """concordance_counts on device-resident uniforms with a coarse array against the torch composition, the two taking turns"""
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    fine = torch.rand((M, n), dtype=torch.float64, device=dev, generator=gen)
    coarse = (fine + 0.02 * torch.randn((M, n), dtype=torch.float64, device=dev, generator=gen)).clamp_(0.0, 1.0)
    fine[0, 5::1001] = float("nan")
    probs = np.array([0.9, 0.95, 0.99])[:G]
    lower, upper = probs[:, None] * np.ones((G, M)), np.full((G, M), np.inf)
    lo_d = torch.from_numpy(lower).to(dev)
    torch.cuda.synchronize()
    ms = np.zeros(2)
    kernel = []

    def entry():
        out = sd.concordance_counts(fine, coarse, lower, upper, device=True, kernel_ms=ms)
        torch.cuda.synchronize()
        kernel.append(ms.copy())
        return out

    def composition():
        keep = ~(torch.isnan(fine).any(dim=0) | torch.isnan(coarse).any(dim=0))
        pair = torch.empty((G, 3, M, M), dtype=torch.float64, device=dev)
        all_ = torch.empty((G, 3), dtype=torch.float64, device=dev)
        for g in range(G):
            ef = ((fine > lo_d[g][:, None]) & keep).to(torch.float64)
            ec = ((coarse > lo_d[g][:, None]) & keep).to(torch.float64)
            # [J^f != J^c] = J^f + J^c - 2 J^f J^c, and sum_j J^f_ab J^c_ab is the Gram of the products e^f_a e^c_a: three Grams
            fc = ef * ec
            gf, gc, both = torch.matmul(ef, ef.T), torch.matmul(ec, ec.T), torch.matmul(fc, fc.T)
            pair[g, 0], pair[g, 1], pair[g, 2] = gf, gc, gf + gc - 2.0 * both
            af, ac = ef.prod(dim=0), ec.prod(dim=0)
            all_[g, 0], all_[g, 1], all_[g, 2] = af.sum(), ac.sum(), (af != ac).sum()
        kept = keep.sum()
        torch.cuda.synchronize()
        return pair, all_, kept

    walls = [[], []]
    for fn in (entry, composition):
        fn()
    kernel.clear()
    for _ in range(reps):
        for k, fn in enumerate((entry, composition)):
            t0 = time.perf_counter()
            fn()
            walls[k].append((time.perf_counter() - t0) * 1e3)
    got, ref = entry(), composition()
    same = bool(torch.equal(got.pair.to(torch.float64), ref[0]) and torch.equal(got.all.to(torch.float64), ref[1])
                and int(got.kept.item()) == int(ref[2].item()))
    k_ms = np.median(np.array(kernel), axis=0)
    rate = 16.0 * M * n / (float(k_ms.sum()) * 1e-3)
    stats = lambda v: dict(min=round(min(v), 3), mean=round(sum(v) / len(v), 3), max=round(max(v), 3))
    return dict(M=M, n=n, G=G, entry_ms=stats(walls[0]), torch_ms=stats(walls[1]),
                torch_over_entry_wall=round(sum(walls[1]) / sum(walls[0]), 2), bits_kernel_ms=round(float(k_ms[0]), 4),
                gram_kernel_ms=round(float(k_ms[1]), 4), tbytes_per_s=round(rate / 1e12, 3), fraction_of_hbm_peak=round(rate / HBM_PEAK, 3),
                equal_torch=same)


def loglik_shape(M, n, dofs, reps, n_host=20_000):
    """copula_log_density on device-resident uniforms with a coarse array, for the models `dofs` at equicorrelation 1/2, against
    the host composition of t_scores with NumPy (on the first n_host columns: SciPy's stdtrit takes about a microsecond per
    value, so the time for n columns is extrapolated and marked so), at G = 1 (Gaussian) also against the torch composition
    ndtri + solve_triangular, the two taking turns; and the t-quantile kernel alone at nu = 3 over M x n values"""
    from scipy import special
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    lo, hi = 2.0 ** -53, 1.0 - 2.0 ** -53
    fine = torch.rand((M, n), dtype=torch.float64, device=dev, generator=gen).clamp_(lo, hi)
    coarse = (fine + 0.02 * torch.randn((M, n), dtype=torch.float64, device=dev, generator=gen)).clamp_(lo, hi)
    corr = np.full((M, M), 0.5)
    np.fill_diagonal(corr, 1.0)
    dofs = np.asarray(dofs, dtype=np.float64)
    G = dofs.size
    models = sd._copula_models("loglik", corr, dofs, M)
    L_d = torch.from_numpy(np.linalg.inv(models.A[0])).to(dev)
    torch.cuda.synchronize()

    def entry():
        out = sd.copula_log_density(fine, corr, dofs, u_coarse=coarse, device=True)
        torch.cuda.synchronize()
        return out

    def torch_gauss():
        out = []
        for u in (fine, coarse):
            y = torch.special.ndtri(u)
            v = torch.linalg.solve_triangular(L_d, y, upper=False)
            out.append(-0.5 * ((v * v).sum(dim=0) - (y * y).sum(dim=0)) - float(models.logdet[0]))
        torch.cuda.synchronize()
        return out

    def quantile_alone():
        out = sd.student_t_quantile(fine, 3.0, device=True)
        torch.cuda.synchronize()
        return out

    nh = min(n, n_host)
    uf_h, uc_h = fine[:, :nh].cpu().numpy(), coarse[:, :nh].cpu().numpy()

    def host():
        out = np.empty((G, 2, nh))
        for g, nu in enumerate(dofs):
            for s, u in enumerate((uf_h, uc_h)):
                z = special.ndtri(u)
                y = z if nu == np.inf else sd.t_scores(z, nu)
                v = models.A[g] @ y
                Q = np.sum(v * v, axis=0)
                if nu == np.inf:
                    out[g, s] = -0.5 * (Q - np.sum(y * y, axis=0)) - models.logdet[g]
                else:
                    cg = special.gammaln(0.5 * (nu + M)) + (M - 1) * special.gammaln(0.5 * nu) - M * special.gammaln(0.5 * (nu + 1.0))
                    out[g, s] = (cg - models.logdet[g] - 0.5 * (nu + M) * np.log1p(Q / nu)
                                 + 0.5 * (nu + 1.0) * np.sum(np.log1p(y * y / nu), axis=0))
        return out

    fns = [entry, quantile_alone] + ([torch_gauss] if G == 1 and dofs[0] == np.inf else [])
    walls = alternating(fns, reps)
    t0 = time.perf_counter()
    ref = host()
    host_ms = (time.perf_counter() - t0) * 1e3
    got = entry()
    err = float(max(np.max(np.abs(got.fine[:, :nh].cpu().numpy() - ref[:, 0])), np.max(np.abs(got.coarse[:, :nh].cpu().numpy() - ref[:, 1]))))
    res = dict(M=M, n=n, G=G, entry_ms=round(walls[0], 3), t_quantile_alone_ms=round(walls[1], 3),
               t_quantile_gvalues_per_s=round(M * n / (walls[1] * 1e-3) / 1e9, 3), host_columns=nh, host_ms_measured=round(host_ms, 1),
               host_ms_extrapolated_to_n=round(host_ms * n / nh, 1), host_over_entry=round(host_ms * n / nh / walls[0], 1),
               max_abs_difference_from_host=err)
    if len(fns) == 3:
        tg = torch_gauss()
        res["torch_ms"] = round(walls[2], 3)
        res["torch_over_entry"] = round(walls[2] / walls[0], 2)
        res["max_abs_difference_from_torch"] = float(max((got.fine[0] - tg[0]).abs().max().item(), (got.coarse[0] - tg[1]).abs().max().item()))
    return res


def single_entries(reps):
    distrs, ok = mixtures(1, 25, seed=5)
    d = distrs[0]
    lam = np.ascontiguousarray(d.multipliers, dtype=np.float64)
    sig = np.ascontiguousarray(d._moment_errs[:len(lam)], dtype=np.float64)
    handle, lib, P = d.moments_fn._basis_handle(), _lib.lib(), _lib.ptr
    x = np.random.default_rng(3).uniform(DOM[0], DOM[1], 10_000_000)
    lo, out = np.full(1_000_000, DOM[0]), np.empty_like(x)
    xd = torch.as_tensor(x[:1_000_000], device="cuda")
    od = torch.empty_like(xd)
    torch.cuda.synchronize()
    ev = lambda xs, os, n, kind: lambda: _lib.check(lib.mlmc_density_eval(handle, P(lam), P(sig), len(lam), P(xs), n, P(os), kind))
    ig = lambda n: lambda: _lib.check(lib.mlmc_density_integrate(handle, P(lam), P(sig), len(lam), P(lo), P(x), n, 21, P(out)))
    res = dict(R1=len(lam), all_success=ok, eval_host_ms={}, eval_device_ms={}, integrate_ms={})
    for n in (1_000, 1_000_000, 10_000_000):
        res["eval_host_ms"][n] = round(timed(ev(x, out, n, _lib.HOST), reps)[0], 4)
    res["eval_device_ms"][1_000_000] = round(timed(ev(xd, od, 1_000_000, _lib.DEVICE), reps)[0], 4)
    for n in (1_000, 1_000_000):
        res["integrate_ms"][n] = round(timed(ig(n), reps)[0], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--config", help="one many-points configuration B,R1,n for a profiler run")
    ap.add_argument("--tails", action="store_true", help="tail_means against quantiles (DESIGN.md section 3.5.9)")
    ap.add_argument("--single", action="store_true", help="the single entries mlmc_density_eval / mlmc_density_integrate")
    ap.add_argument("--divergences", action="store_true", help="divergences against host sums and quad (DESIGN.md section 3.5.10)")
    ap.add_argument("--moments", action="store_true", help="density_moments against host sums (DESIGN.md section 3.5.11)")
    ap.add_argument("--samples", action="store_true", help="samples against torch.rand + quantiles (DESIGN.md section 3.5.12)")
    ap.add_argument("--joint", action="store_true", help="joint_samples against samples and torch.randn + matmul + ndtr + quantiles "
                                                         "(DESIGN.md section 3.5.13)")
    ap.add_argument("--tcopula", action="store_true", help="joint_samples(dof=3, 30) against the Gaussian entry of the same shape, and "
                                                           "the map and mixing functions on their own (DESIGN.md section 3.5.22)")
    ap.add_argument("--scores", action="store_true", help="normal_scores against cdfs_on_rule + torch ndtri, and estimate_score_correlation "
                                                          "against estimate_component_covariance (DESIGN.md section 3.5.14)")
    ap.add_argument("--conditional", action="store_true", help="conditional_samples of B sets against a loop of single-set calls and "
                                                               "joint_samples of as many draws (DESIGN.md section 3.5.15)")
    ap.add_argument("--tconditional", action="store_true", help="conditional_samples(dof=3, 30) against the Gaussian conditional_samples "
                    "of the same shape, and the map and mixing functions on their own (DESIGN.md section 3.5.24)")
    ap.add_argument("--qmc", action="store_true", help="samples / joint_samples / conditional_samples with and without qmc, and the RMS "
                                                       "error of two integrals against n (DESIGN.md section 3.5.16)")
    ap.add_argument("--boxprob", action="store_true", help="copula_box_probabilities against closed forms, next to counting the "
                                                           "scenarios of joint_samples (DESIGN.md section 3.5.17)")
    ap.add_argument("--boxdraws", action="store_true", help="event_samples against rejection from joint_samples (DESIGN.md section 3.5.18)")
    ap.add_argument("--tboxprob", action="store_true", help="copula_box_probabilities / event_samples with dof = 3, 30 against the Gaussian "
                    "calls of the same shapes (DESIGN.md section 3.5.23)")
    ap.add_argument("--tcondbox", action="store_true", help="conditional_box_probabilities / conditional_box_draws (p = 1, B in {1, 64} sets) "
                    "against the t entries of the same shapes (DESIGN.md section 3.5.26)")
    ap.add_argument("--tlead", action="store_true", help='copula_box_probabilities(dof = 3, 30, mixing="conditioned") against the plain t '
                    "call of the same shapes: time, prob, stderr and ess / n of both (DESIGN.md section 3.5.27)")
    ap.add_argument("--boxorder", action="store_true", help="box_order alone, the reordered chain call against the natural one, and the "
                    "one-call bands against the loop of calls (DESIGN.md section 3.5.28)")
    ap.add_argument("--aggregates", action="store_true", help="mlmc_scenario_aggregates against the torch composition on a materialised "
                                                              "scenario matrix (DESIGN.md section 3.5.20)")
    ap.add_argument("--concordance", action="store_true", help="concordance_counts against the torch composition of indicator matrices and "
                                                               "fp64 Grams (DESIGN.md section 3.5.21)")
    ap.add_argument("--loglik", action="store_true", help="copula_log_density with the default grid of nu and with the Gaussian model alone "
                    "against the host composition of t_scores with NumPy and the torch composition, and the t-quantile kernel alone "
                    "(DESIGN.md section 3.5.25)")
    ap.add_argument("--reps", type=int, default=None)
    a = ap.parse_args()
    if a.reps is None:
        a.reps = 5 if a.concordance or a.tcopula or a.tconditional else 3
    _lib.init(0)
    out = dict(tool="quantile_batch", device=_lib.device_info()["name"])
    if a.single:
        out["single"] = single_entries(a.reps)
    elif a.loglik:
        shapes = [(12, 1_000_000), (64, 100_000)]
        if a.config:
            shapes = [tuple(int(v) for v in a.config.split(","))]
        elif a.quick:
            shapes = [(4, 10_000)]
        out["loglik"] = [loglik_shape(M, n, dofs, a.reps, n_host=2_000 if a.quick else 20_000)
                         for M, n in shapes for dofs in (sd.COPULA_DOF_GRID, (np.inf,))]
    elif a.concordance:
        shapes = [(12, 1_000_000), (64, 1_000_000), (256, 100_000)]
        if a.config:
            shapes = [tuple(int(v) for v in a.config.split(","))]
        elif a.quick:
            shapes = [(12, 10_000), (5, 1_000)]
        out["concordance"] = [concordance_shape(M, n, a.reps) for M, n in shapes]
    elif a.aggregates:
        shapes = [(1, 12, 1_000_000), (1, 64, 1_000_000), (64, 12, 10_000)]
        if a.config:
            shapes = [tuple(int(v) for v in a.config.split(","))]
        elif a.quick:
            shapes = [(1, 12, 10_000), (3, 5, 1_000)]
        _lib.use_torch_stream()
        out["aggregates"] = [aggregates_shape(S, M, n, a.reps) for S, M, n in shapes]
    elif a.boxorder:
        kernel = [(M, B) for M in (12, 64, 128) for B in (1, 64, 300)]
        calls = [(12, 1, 2 ** 12), (12, 64, 2 ** 12), (12, 300, 2 ** 12), (64, 64, 2 ** 12), (12, 1, 2 ** 16)]
        bands = [(12, 300, 2 ** 12)]
        if a.quick:
            kernel, calls, bands = [(12, 3), (65, 2)], [(12, 3, 2 ** 10)], [(3, 8, 2 ** 10)]
        out["boxorder_kernel"] = [boxorder_kernel_shape(M, B, a.reps) for M, B in kernel]
        out["boxorder_call"] = [boxorder_call_shape(M, B, n, a.reps) for M, B, n in calls]
        out["boxorder_bands"] = [boxorder_bands_shape(M, B, n, a.reps) for M, B, n in bands]
    elif a.tlead:
        t6 = brentq(lambda t: np.log(equicorrelated_exceedance(12, t)) - np.log(1e-6), 0.0, 6.0, xtol=1e-10)
        shapes = [(M, 1, 2 ** k, 0.0) for M in (2, 12, 64) for k in (12, 16, 20)] + [(M, 64, 2 ** k, 0.0) for M in (2, 12, 64) for k in (12, 16)]
        shapes += [(12, 1, 2 ** k, t6) for k in (12, 16, 20)]
        if a.config:
            M, n = (int(v) for v in a.config.split(","))
            shapes = [(M, 1, n, 0.0)]
        elif a.quick:
            shapes = [(2, 1, 2 ** 12, 0.0), (2, 64, 2 ** 12, 0.0), (12, 3, 2 ** 12, t6)]
        out["tlead"] = [tlead_shape(M, B, n, a.reps, t, dof) for M, B, n, t in shapes for dof in (3.0, 30.0)]
    elif a.tcondbox:
        t6 = brentq(lambda t: np.log(equicorrelated_exceedance(12, t)) - np.log(1e-6), 0.0, 6.0, xtol=1e-10)
        shapes = [(M, 1, 2 ** k, 0.0) for M in (2, 12, 64) for k in (12, 16, 20)] + [(M, 64, 2 ** k, 0.0) for M in (2, 12, 64) for k in (12, 16)]
        shapes += [(12, 1, 2 ** k, t6) for k in (12, 16, 20)]
        draws = [(M, 1, 2 ** k) for M in (2, 12, 64) for k in (12, 16)] + [(M, 64, 2 ** 12) for M in (2, 12)]
        if a.config:
            M, n = (int(v) for v in a.config.split(","))
            shapes, draws = [(M, 1, n, 0.0)], [(M, 1, n)]
        elif a.quick:
            shapes, draws = [(2, 1, 2 ** 12, 0.0), (12, 64, 2 ** 12, t6)], [(2, 1, 2 ** 12), (12, 64, 2 ** 12)]
        out["tcondbox"] = [tcondbox_shape(M, B, n, a.reps, t, dof) for M, B, n, t in shapes for dof in (3.0, 30.0)]
        out["tcondbox_draws"] = [tcondbox_shape(M, B, n, a.reps, 0.0, dof, draws=True) for M, B, n in draws for dof in (3.0, 30.0)]
    elif a.tboxprob:
        t6 = brentq(lambda t: np.log(equicorrelated_exceedance(12, t)) - np.log(1e-6), 0.0, 6.0, xtol=1e-10)
        shapes = [(M, 1, 2 ** k, 0.0) for M in (2, 12, 64) for k in (12, 16, 20)] + [(M, 64, 2 ** k, 0.0) for M in (2, 12, 64) for k in (12, 16)]
        shapes += [(12, 1, 2 ** k, t6) for k in (12, 16, 20)]
        draws = [(M, 2 ** k, 0.9) for M in (2, 12, 64) for k in (12, 16, 20)] + [(12, 2 ** k, 0.999) for k in (12, 16, 20)]
        if a.config:
            M, n = (int(v) for v in a.config.split(","))
            shapes, draws = [(M, 1, n, 0.0)], [(M, n, 0.9)]
        elif a.quick:
            shapes, draws = [(2, 1, 2 ** 12, 0.0), (12, 3, 2 ** 12, t6)], [(2, 2 ** 12, 0.9), (12, 2 ** 12, 0.999)]
        out["tboxprob"] = [tboxprob_shape(M, B, n, a.reps, t, dof) for M, B, n, t in shapes for dof in (3.0, 30.0)]
        out["tboxdraws"] = [tboxdraws_shape(M, n, a.reps, p, dof) for M, n, p in draws for dof in (3.0, 30.0)]
    elif a.boxdraws:
        shapes = [(M, 2 ** k, 0.9) for M in (2, 12, 64) for k in (12, 16, 20)] + [(12, 2 ** k, 0.999) for k in (12, 16, 20)]
        if a.config:
            M, n = (int(v) for v in a.config.split(","))
            shapes = [(M, n, 0.9)]
        elif a.quick:
            shapes = [(2, 2 ** 12, 0.9), (12, 2 ** 12, 0.999)]
        out["boxdraws"] = [boxdraws_shape(M, n, a.reps, p) for M, n, p in shapes]
    elif a.boxprob:
        # the orthant under equicorrelation 1/2, and for M = 12 the threshold at which all twelve exceed it with probability 1e-6
        t6 = brentq(lambda t: np.log(equicorrelated_exceedance(12, t)) - np.log(1e-6), 0.0, 6.0, xtol=1e-10)
        shapes = [(M, 1, 2 ** k, 0.0) for M in (2, 12, 64) for k in (12, 16, 20)] + [(M, 64, 2 ** k, 0.0) for M in (2, 12, 64) for k in (12, 16)]
        shapes += [(12, 1, 2 ** k, t6) for k in (12, 16, 20)]
        if a.config:
            M, B, n = (int(v) for v in a.config.split(","))
            shapes = [(M, B, n, 0.0)]
        elif a.quick:
            shapes = [(2, 1, 2 ** 12, 0.0), (12, 3, 2 ** 12, 0.0), (12, 1, 2 ** 12, t6)]
        out["boxprob"] = [boxprob_shape(M, B, n, a.reps, t) for M, B, n, t in shapes]
    elif a.qmc:
        out["qmc_times"] = qmc_times(a.reps, a.quick)
        out["qmc_errors"] = qmc_errors(a.quick)
    elif a.tconditional:
        shapes = [(12, 25, 1, 1_000_000), (12, 25, 64, 10_000), (12, 25, 1024, 1_000)]
        if a.config:
            shapes = [tuple(int(v) for v in a.config.split(","))]
        elif a.quick:
            shapes = [(4, 9, 3, 1_000)]
        out["tconditional"] = [tconditional_shape(M, R1, B, n, dof, a.reps) for M, R1, B, n in shapes for dof in (3.0, 30.0)]
    elif a.conditional:
        shapes = [(12, 25, 1, 1_000_000), (12, 25, 64, 10_000), (12, 25, 1024, 1_000)]
        if a.config:
            shapes = [tuple(int(v) for v in a.config.split(","))]
        elif a.quick:
            shapes = [(4, 9, 3, 1_000)]
        out["conditional"] = [conditional_shape(M, R1, B, n, a.reps) for M, R1, B, n in shapes]
    elif a.scores:
        shapes = [(12, 25, 1_000_000, 5), (64, 25, 1_000_000, 0), (256, 25, 100_000, 0)]
        if a.config:
            shapes = [tuple(int(v) for v in a.config.split(","))]
        elif a.quick:
            shapes = [(4, 9, 10_000, 2)]
        out["scores"] = [scores_shape(M, R1, n, a.reps, levels) for M, R1, n, levels in shapes]
    elif a.tcopula:
        shapes = [(12, 25, 1_000_000, 12), (64, 25, 1_000_000, 64), (256, 25, 100_000, 256)]
        if a.config:
            shapes = [tuple(int(v) for v in a.config.split(","))]
        elif a.quick:
            shapes = [(4, 9, 10_000, 4)]
        out["tcopula"] = [tcopula_shape(M, R1, n, K, dof, a.reps) for M, R1, n, K in shapes for dof in (3.0, 30.0)]
    elif a.joint:
        shapes = [(12, 25, 1_000_000, 12), (64, 25, 1_000_000, 64), (256, 25, 100_000, 256), (12, 25, 1_000_000, 3)]
        if a.config:
            shapes = [tuple(int(v) for v in a.config.split(","))]
        elif a.quick:
            shapes = [(4, 9, 10_000, 4)]
        out["joint"] = [joint_shape(M, R1, n, K, a.reps) for M, R1, n, K in shapes]
    elif a.samples:
        shapes = [(1, 9, 10_000_000), (1, 25, 10_000_000), (1, 64, 10_000_000), (64, 25, 1_000_000), (3600, 25, 1_000)]
        if a.config:
            shapes = [tuple(int(v) for v in a.config.split(","))]
        elif a.quick:
            shapes = [(4, 9, 10_000)]
        out["samples"] = [samples_shape(B, R1, n, a.reps) for B, R1, n in shapes]
    elif a.moments:
        out["moments"] = [moments_batch(B, a.reps) for B in ((16,) if a.quick else (16, 3600, 19200))]
    elif a.divergences:
        shapes = ((16, 1),) if a.quick else ((16, 1), (300, 12), (300, 64))
        out["divergences"] = [divergence_pairs(n_rep, n_comp, a.reps) for n_rep, n_comp in shapes]
    elif a.tails:
        cfg = tuple(int(v) for v in a.config.split(",")) if a.config else (1, 25, 1_000_000)
        if not a.config:
            Ms = (16,) if a.quick else (16, 256, 1024)
            out["tails_few"] = [tails_few_points(M, probs, a.reps) for M in Ms
                                for probs in (np.array([0.05, 0.5, 0.95]), np.linspace(0.01, 0.99, 99))]
        out["tails_many"] = [tails_many_points(*cfg, a.reps)]
    elif a.config:
        B, R1, n = (int(v) for v in a.config.split(","))
        out["many"] = [many_points(B, R1, n, a.reps)]
    else:
        Ms = (16,) if a.quick else (16, 64, 256, 1024)
        out["few"] = [few_points(M, probs, a.reps) for M in Ms for probs in (np.array([0.05, 0.5, 0.95]), np.linspace(0.01, 0.99, 99))]
        cfgs = [(1, 25, 1_000_000)] if a.quick else [(B, R1, n) for n in (1_000_000, 10_000_000) for R1 in (9, 25, 64) for B in (1, 8, 64)]
        out["many"] = [many_points(B, R1, n, a.reps) for B, R1, n in cfgs]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
