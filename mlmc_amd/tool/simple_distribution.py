"""Maximum-entropy PDF from generalised moments (reference interface: mlmc/tool/simple_distribution.py).

`SimpleDistribution`, `construct_ortogonal_moments` and the diagnostic integrals keep the reference's names,
arguments and result fields.  The optimisation itself (functional, gradient, Hessian on a quadrature, Newton
steps with a Cholesky solve) runs on the MI355X through `mlmc_maxent_solve`; `density` and `cdf` are device
kernels as well.  The reference's SciPy trust-ncg iterates and QUADPACK sub-interval layout are not reproduced
(they are pinned by no reference test); the converged multipliers are, because the functional is
strictly convex.
"""
import collections
import ctypes as C

import numpy as np
import scipy.integrate as integrate
import scipy.linalg


class _SmallLapack:
    """Context for the dense LAPACK calls of this module (eigh, rq, eigvalsh on matrices of at most 128 x 128): one BLAS
    thread.  On a many-core host the threaded BLAS spreads such a call over every core it sees -- on the MI355X boxes of this
    pool (256 logical cores, a 16-core share per GPU) a 128 x 128 `eigh` that takes 3 ms on one thread took 85-90 ms, thirty
    times the GPU part of construct_density.  threadpoolctl is optional: without it the calls run as NumPy configures them."""
    _controller = None

    def __enter__(self):
        self._ctx = None
        try:
            if _SmallLapack._controller is None:
                from threadpoolctl import ThreadpoolController
                _SmallLapack._controller = ThreadpoolController()
            self._ctx = _SmallLapack._controller.limit(limits=1, user_api="blas")
            self._ctx.__enter__()
        except Exception:
            self._ctx = None
        return self

    def __exit__(self, *exc):
        if self._ctx is not None:
            self._ctx.__exit__(*exc)
        return False

from scipy.optimize import OptimizeResult

from .. import _lib
from .. import moments as moments_mod

EXACT_QUAD_LIMIT = 1000


def _solve_on_device(moments_fn, means, errs, domain, multipliers, tol, max_it, n_intervals=0, gauss_degree=21,
                     stab_penalty=0.0, penalty_coef=0.0, decay=(False, False), prev=None):
    size = len(multipliers)
    opts = _lib.MaxentOpts()
    opts.tol = float(tol)
    opts.max_it = int(max_it)
    opts.n_intervals = int(n_intervals)
    opts.gauss_degree = int(gauss_degree)
    opts.stab_penalty = float(stab_penalty)
    opts.penalty_coef = float(penalty_coef)
    opts.decay_left, opts.decay_right = int(bool(decay[0])), int(bool(decay[1]))
    info = _lib.MaxentInfo()
    lam = np.ascontiguousarray(multipliers, dtype=np.float64).copy()
    mu = np.ascontiguousarray(means[:size], dtype=np.float64)
    sig = np.ascontiguousarray(errs[:size], dtype=np.float64)
    hess = np.empty((size, size), dtype=np.float64)
    grad = np.empty(size, dtype=np.float64)
    prev_arr = None if prev is None else np.ascontiguousarray(prev, dtype=np.float64)
    _lib.check(_lib.lib().mlmc_maxent_solve(moments_fn._basis_handle(), _lib.ptr(mu), _lib.ptr(sig), size, float(domain[0]),
                                            float(domain[1]), C.byref(opts), _lib.ptr(prev_arr),
                                            0 if prev_arr is None else len(prev_arr), _lib.ptr(lam), _lib.ptr(grad), _lib.ptr(hess), C.byref(info)))
    return lam, grad, hess, info


def _solve_batch_on_device(moments_fns, means, errs, domains, multipliers, tol, max_it, n_intervals=0, gauss_degree=21):
    """B problems of _solve_on_device's functional (no penalties) in one mlmc_maxent_solve_batch call.
    means / errs / multipliers: sequences of B vectors (problem b uses the first len(multipliers[b]) entries).
    :return: list of (lam, grad, hess, info) per problem, as _solve_on_device returns them"""
    B = len(moments_fns)
    if B == 0:
        return []
    r1 = np.array([len(m) for m in multipliers], dtype=np.int32)
    ldv = int(r1.max())
    mu = np.zeros((B, ldv))
    sig = np.ones((B, ldv))
    lam = np.zeros((B, ldv))
    for b in range(B):
        r = r1[b]
        mu[b, :r] = np.asarray(means[b], dtype=np.float64)[:r]
        sig[b, :r] = np.asarray(errs[b], dtype=np.float64)[:r]
        lam[b, :r] = np.asarray(multipliers[b], dtype=np.float64)
    lo = np.ascontiguousarray([float(d[0]) for d in domains], dtype=np.float64)
    hi = np.ascontiguousarray([float(d[1]) for d in domains], dtype=np.float64)
    opts = _lib.MaxentOpts()
    opts.tol = float(tol)
    opts.max_it = int(max_it)
    opts.n_intervals = int(n_intervals)
    opts.gauss_degree = int(gauss_degree)
    handles = (C.c_void_p * B)(*[fn._basis_handle().value for fn in moments_fns])
    infos = (_lib.MaxentInfo * B)()
    grad = np.empty((B, ldv))
    hess = np.empty((B, ldv, ldv))
    _lib.check(_lib.lib().mlmc_maxent_solve_batch(B, C.cast(handles, C.c_void_p), _lib.ptr(r1), _lib.ptr(lo), _lib.ptr(hi),
                                                  _lib.ptr(mu), _lib.ptr(sig), C.byref(opts), _lib.ptr(lam), _lib.ptr(grad),
                                                  _lib.ptr(hess), C.cast(infos, C.c_void_p)))
    return [(lam[b, :r1[b]].copy(), grad[b, :r1[b]].copy(), hess[b, :r1[b], :r1[b]].copy(), infos[b]) for b in range(B)]


def densities(distrs, values):
    """density() of many distributions in one device launch (mlmc_density_eval_batch).
    values: one array of points for all (broadcast) or a sequence with one array per distribution.
    :return: list of arrays, entry b = distrs[b].density(values[b]) bit for bit"""
    B = len(distrs)
    if B == 0:
        return []
    if isinstance(values, np.ndarray) or np.isscalar(values) or (len(values) > 0 and np.isscalar(values[0])):
        values = [values] * B
    shaped = [np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in values]
    flat = np.ascontiguousarray(np.concatenate([v.reshape(-1) for v in shaped]))
    n = np.array([v.size for v in shaped], dtype=np.int64)
    r1 = np.array([len(d.multipliers) for d in distrs], dtype=np.int32)
    ldv = int(r1.max())
    lam = np.zeros((B, ldv))
    sig = np.ones((B, ldv))
    for b, d in enumerate(distrs):
        lam[b, :r1[b]] = d.multipliers
        sig[b, :r1[b]] = d._moment_errs[:r1[b]]
    out = np.empty_like(flat)
    handles = (C.c_void_p * B)(*[d.moments_fn._basis_handle().value for d in distrs])
    _lib.check(_lib.lib().mlmc_density_eval_batch(B, C.cast(handles, C.c_void_p), _lib.ptr(r1), _lib.ptr(lam), _lib.ptr(sig),
                                                  _lib.ptr(flat), _lib.ptr(n), _lib.ptr(out)))
    parts = np.split(out, np.cumsum(n)[:-1])
    return [p.reshape(v.shape) for p, v in zip(parts, shaped)]


def _per_distribution(values, B):
    """one entry per distribution from `values`: one 1-D array / scalar / flat sequence for all, or a sequence of B arrays.  An array
    of more than one dimension is ambiguous ([B, n] rows per distribution, or one block for all?) and raises: pass list(array) for
    rows, array.ravel() for one block."""
    if (isinstance(values, np.ndarray) or hasattr(values, "data_ptr")) and values.ndim > 1:
        raise ValueError("an array of {} dimensions is ambiguous: pass a list with one array per distribution, or one 1-D "
                         "array for all".format(values.ndim))
    if isinstance(values, np.ndarray) or hasattr(values, "data_ptr") or np.isscalar(values) \
            or (len(values) > 0 and np.isscalar(values[0])):
        return [values] * B
    if len(values) != B:
        raise ValueError("{} arrays for {} distributions".format(len(values), B))
    return list(values)


def _batch_problem_args(distrs):
    """(handles, r1, lam, sig) of a list of distributions in the layout of the batched density entry points"""
    B = len(distrs)
    r1 = np.array([len(d.multipliers) for d in distrs], dtype=np.int32)
    ldv = int(r1.max())
    lam = np.zeros((B, ldv))
    sig = np.ones((B, ldv))
    for b, d in enumerate(distrs):
        lam[b, :r1[b]] = d.multipliers
        sig[b, :r1[b]] = d._moment_errs[:r1[b]]
    handles = (C.c_void_p * B)(*[d.moments_fn._basis_handle().value for d in distrs])
    return handles, r1, lam, sig


def _common_quadrature(what, distrs):
    """(n_intervals, Gauss degree) of a non-empty list of distributions, which must all use the same"""
    n_int = {d.n_intervals for d in distrs}
    degs = {d._gauss_degree for d in distrs}
    if len(n_int) != 1 or len(degs) != 1:
        raise ValueError(what + ": every distribution must use the same quadrature")
    return int(n_int.pop()), int(degs.pop())


def _domain_arrays(distrs):
    """(a [B], b [B]): the ends of the distributions' domains in the layout of the batched density entry points"""
    a = np.ascontiguousarray([float(d.domain[0]) for d in distrs], dtype=np.float64)
    b = np.ascontiguousarray([float(d.domain[1]) for d in distrs], dtype=np.float64)
    return a, b


def _check_seed(what, seed):
    if seed is None or isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
        raise ValueError(what + ": seed must be an integer in 0 .. 2^64 - 1")


def _checked_streams(what, streams, count, per):
    """None, or `streams` as a uint32 array [count]; `per` says in the message what has a stream of its own"""
    if streams is None:
        return None
    st = np.asarray(streams)
    if st.shape != (count,) or (st.size and (st.dtype.kind not in "iu" or np.any(st < 0) or np.any(st.astype(np.uint64) >= 2 ** 32))):
        raise ValueError("{}: streams must be one integer in 0 .. 2^32 - 1 per {}".format(what, per))
    return np.ascontiguousarray(st.astype(np.uint32))


def _output_arrays(device, shapes):
    """float64 arrays of the given shapes (None: no array) for the library to write, and their memory kind: NumPy arrays, or
    (device) tensors on the current device, made before a synchronise of its current stream, since the library writes them on
    its own stream"""
    if not device:
        return [None if s is None else np.empty(s) for s in shapes], _lib.HOST
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    arrays = [None if s is None else torch.empty(s, dtype=torch.float64, device=dev) for s in shapes]
    torch.cuda.current_stream(dev).synchronize()
    return arrays, _lib.DEVICE


def cdfs(distrs, values):
    """cdf() of many distributions through ONE device call (mlmc_density_integrate_batch).
    values: one array of points for all or a sequence with one array per distribution, as in `densities`.
    :return: list of arrays, entry b = distrs[b].cdf(values[b]) bit for bit: the cumulative 10-point pieces between successive
        in-domain values, prefix-summed on the host in the order of `_cdf` (values outside the domain and unsorted values behave
        as there; like cdf() it takes no NaN values -- `cdfs_on_rule` does)"""
    B = len(distrs)
    if B == 0:
        return []
    vals = [np.atleast_1d(v) for v in _per_distribution(values, B)]
    lo, hi = [], []
    n = np.zeros(B, dtype=np.int64)
    for b, (d, v) in enumerate(zip(distrs, vals)):
        last_x = d.domain[0]
        for val in v:
            if d.domain[0] < val < d.domain[1]:
                lo.append(last_x)
                hi.append(val)
                last_x = val
                n[b] += 1
    lo = np.ascontiguousarray(lo, dtype=np.float64)
    hi = np.ascontiguousarray(hi, dtype=np.float64)
    pieces = np.empty_like(lo)
    handles, r1, lam, sig = _batch_problem_args(distrs)
    _lib.check(_lib.lib().mlmc_density_integrate_batch(B, C.cast(handles, C.c_void_p), _lib.ptr(r1), _lib.ptr(lam), _lib.ptr(sig),
                                                       _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(n), 10, _lib.ptr(pieces)))
    out, k = [], 0
    for d, v in zip(distrs, vals):
        cdf_y = np.empty(len(v))
        last_y = 0
        for i, val in enumerate(v):
            if val <= d.domain[0]:
                last_y = 0
            elif val >= d.domain[1]:
                last_y = 1
            else:
                last_y = last_y + pieces[k]
                k += 1
            cdf_y[i] = last_y
        out.append(cdf_y)
    return out


def _on_rule(distrs, points, inverse, what, tails=False):
    """mlmc_density_quantiles_batch (inverse) / mlmc_density_cdf_batch / mlmc_density_tail_means_batch (tails) of a list of
    distributions in ONE call.
    points: per distribution a NumPy-convertible array, or torch device tensors for all of them (float64; the results are
    device tensors then and nothing is copied to the host).
    :return: (list of arrays shaped like the points, masses [B]); with tails ((q, lower, upper, means [B]), masses [B]), q, lower
        and upper each such a list"""
    B = len(distrs)
    n_int, deg = _common_quadrature(what, distrs)
    on_device = [hasattr(p, "data_ptr") and p.is_cuda for p in points]
    handles, r1, lam, sig = _batch_problem_args(distrs)
    a, b = _domain_arrays(distrs)
    mass = np.empty(B)
    if any(on_device):
        import torch
        if not all(on_device) or any(p.dtype != torch.float64 for p in points):
            raise ValueError(what + ": device points must be float64 device tensors for every distribution")
        shaped = list(points)
        flat = shaped[0].contiguous().reshape(-1) if B == 1 else torch.cat([p.reshape(-1) for p in shaped])
        outs = [torch.empty_like(flat) for _ in range(3 if tails else 1)]
        n = np.array([p.numel() for p in shaped], dtype=np.int64)
        torch.cuda.current_stream(flat.device).synchronize()         # the library reads it on its own stream
        kind = _lib.DEVICE
    else:
        shaped = [np.atleast_1d(np.asarray(p, dtype=np.float64)) for p in points]
        flat = np.ascontiguousarray(np.concatenate([p.reshape(-1) for p in shaped]))
        outs = [np.empty_like(flat) for _ in range(3 if tails else 1)]
        n = np.array([p.size for p in shaped], dtype=np.int64)
        kind = _lib.HOST
    head = (B, C.cast(handles, C.c_void_p), _lib.ptr(r1), _lib.ptr(lam), _lib.ptr(sig), _lib.ptr(a), _lib.ptr(b),
            n_int, deg, _lib.ptr(flat), _lib.ptr(n))
    if tails:
        mean = np.empty(B)
        _lib.check(_lib.lib().mlmc_density_tail_means_batch(*head, _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]),
                                                            _lib.ptr(mass), _lib.ptr(mean), kind))
    else:
        fn = _lib.lib().mlmc_density_quantiles_batch if inverse else _lib.lib().mlmc_density_cdf_batch
        _lib.check(fn(*head, _lib.ptr(outs[0]), _lib.ptr(mass), kind))

    def per_distribution(out):
        if kind == _lib.DEVICE:
            import torch
            parts = [out] if B == 1 else list(torch.split(out, [int(k) for k in n]))
        else:
            parts = np.split(out, np.cumsum(n)[:-1])
        return [p.reshape(s.shape) for p, s in zip(parts, shaped)]
    if tails:
        return (per_distribution(outs[0]), per_distribution(outs[1]), per_distribution(outs[2]), mean), mass
    return per_distribution(outs[0]), mass


def cdfs_on_rule(distrs, values):
    """Fhat of many distributions through ONE device call (mlmc_density_cdf_batch): the normalised CDF on each distribution's
    own quadrature (n_intervals cells of _gauss_degree points), the function that `quantiles` inverts.  With the cell edges
    e_j, the cell integrals C_j, their in-order prefix P_j and the mass T = P_n (include/mlmc_hip.h),
        Fhat(x) = (P_j + I(e_j, x)) / T for x in cell j, 0 for x <= a, 1 for x >= b, NaN for NaN.
    Unlike `cdfs` every value is evaluated on its own: the result does not depend on the order of `values`, and it is
    normalised by the mass of the rule (Fhat(b) = 1 exactly).
    values: one array for all or one per distribution.  :return: list of arrays"""
    distrs = list(distrs)
    if not distrs:
        return []
    return _on_rule(distrs, _per_distribution(values, len(distrs)), False, "cdfs_on_rule")[0]


def quantiles(distrs, probs):
    """Quantiles of many distributions through ONE device call (mlmc_density_quantiles_batch): entry b = Q_b(probs[b]), the x in
    the domain with Fhat_b(x) = p (`cdfs_on_rule`); Q(0) and Q(1) are the domain's end points exactly, p outside [0, 1] or NaN
    gives NaN (SciPy's ppf convention).  A value is bit for bit the same for a distribution alone or in any batch.
    probs: one array for all or one per distribution; every distribution uses its own n_intervals / _gauss_degree, which must
    agree over the list (ValueError otherwise).  :return: list of arrays"""
    distrs = list(distrs)
    if not distrs:
        return []
    return _on_rule(distrs, _per_distribution(probs, len(distrs)), True, "quantiles")[0]


def tail_means(distrs, probs):
    """Quantiles and tail means (expected shortfall, CVaR) of many distributions through ONE device call
    (mlmc_density_tail_means_batch).  With Q = `quantiles` and the rule of `cdfs_on_rule`, entry b of
        q     = Q_b(probs[b]), bit for bit the value of `quantiles`,
        lower = E[X | X <= q], the lower expected shortfall at level p,
        upper = E[X | X >= q], the upper one,
    each a mean of the density on the distribution's own quadrature, normalised by the mass of the tail on the same rule
    (include/mlmc_hip.h); lower(Q(0)) = a, upper(Q(1)) = b, NaN for p outside [0, 1] or NaN; mean [B] is the mean of every
    distribution on its rule.  p lower + (1 - p) upper equals the mean only up to the resolution of the rule.
    probs: as in `quantiles` (one array for all or one per distribution, a common quadrature or ValueError; float64 device
    tensors stay on the device).  :return: (q, lower, upper, mean): three lists of arrays shaped like the probabilities, mean [B]"""
    distrs = list(distrs)
    if not distrs:
        return [], [], [], np.empty(0)
    return _on_rule(distrs, _per_distribution(probs, len(distrs)), True, "tail_means", tails=True)[0]


def _expected_shortfall(dist, p, tail):
    """the B = 1 call of `tail_means`: upper(Q(p)) or lower(Q(p)); a torch device tensor stays on the device"""
    if tail not in ("upper", "lower"):
        raise ValueError("expected_shortfall: tail must be 'upper' or 'lower', got {!r}".format(tail))
    _, lower, upper, _ = _on_rule([dist], [p], True, "expected_shortfall", tails=True)[0]
    return upper[0] if tail == "upper" else lower[0]


def _quantile(dist, p):
    """the B = 1 call of `quantiles`; a torch device tensor stays on the device"""
    res = _on_rule([dist], [p], True, "quantile")[0][0]
    return res


def _per_distribution_int(what, name, value, B):
    """[B] int64 from one integer for all or one per distribution"""
    arr = np.asarray(value)
    if arr.ndim > 1 or (arr.ndim == 1 and arr.size != B):
        raise ValueError("{}: {} must be one integer or one per distribution".format(what, name))
    if arr.dtype.kind not in "iu" or np.any(arr < 0) or np.any(arr.astype(np.uint64) > np.uint64(2 ** 63 - 1)):
        raise ValueError("{}: {} must be non-negative integers below 2^63".format(what, name))
    return np.ascontiguousarray(np.broadcast_to(arr.astype(np.int64), (B,)))


def samples(distrs, n, seed, streams=None, first=0, antithetic=False, device=False, return_uniforms=False, qmc=False):
    """Seeded draws from many distributions through ONE device call (mlmc_density_sample_batch): inverse-transform sampling on
    each distribution's quadrature.  Draw j of stream s under `seed` is Q(u_j) with Q of `quantiles` (bit for bit its value at
    p = u_j) and u_j the Philox4x32-10 uniform that include/mlmc_hip.h defines, an odd multiple of 2^-53 in (0, 1).  Entry b holds
    the draws first[b] .. first[b] + n[b] - 1 of stream streams[b].  A draw depends on (seed, stream, j, antithetic, distribution,
    quadrature) alone: not on n, on first or on the other distributions, so `first` continues a run and streams (or ranges of
    j) split it across ranks.  The draws of different distributions are independent unless they are given one stream.
    :param n: draws per distribution, one int for all or one per distribution
    :param seed: required, 0 <= seed < 2^64; there is no global generator
    :param streams: one uint32 stream per distribution; default: stream b = b
    :param first: index of the first draw, one int for all or one per distribution
    :param antithetic: draws 2k and 2k + 1 come from u and 1 - u
    :param qmc: randomised quasi-Monte Carlo (MLMC_SAMPLE_SOBOL): u_j is coordinate `stream` of point j of the scrambled Sobol'
        sequence of include/mlmc_hip.h instead of the Philox uniform.  The streams are then DIMENSIONS and must be below 1024; n
        should be a power of two and `first` a multiple of it, since the points are balanced over blocks aligned to powers of two
        (any first and n are allowed).  For an error bar repeat with R seeds: the seeds give independent scrambles, and the sample
        standard deviation of the R means estimates the error of their mean.  Not together with antithetic
    :param device: return float64 torch device tensors; nothing but the problem table touches the host then
    :param return_uniforms: also return the list of the u_j
    :return: list of arrays [n[b]] (and the same list of uniforms); every distribution must use the same quadrature"""
    out, u, n = _samples_flat(distrs, n, seed, streams, first, antithetic, device, return_uniforms, qmc)

    def per_distribution(flat):
        if device:
            import torch
            return list(torch.split(flat, [int(k) for k in n]))
        return np.split(flat, np.cumsum(n)[:-1])
    if out is None:
        return ([], []) if return_uniforms else []
    return (per_distribution(out), per_distribution(u)) if return_uniforms else per_distribution(out)


def _sample_flags(what, antithetic, qmc):
    """the flags word of a sampling entry; qmc with antithetic is an error before anything touches the device"""
    if qmc and antithetic:
        raise ValueError(what + ": qmc and antithetic exclude each other")
    return (_lib.SAMPLE_ANTITHETIC if antithetic else 0) | (_lib.SAMPLE_SOBOL if qmc else 0)


def _samples_flat(distrs, n, seed, streams, first, antithetic, device, return_uniforms, qmc=False):
    """the call behind `samples`: (draws, uniforms or None, counts [B]) with the distributions' draws one after another in one
    array or device tensor; (None, None, counts) for an empty list"""
    distrs = list(distrs)
    B = len(distrs)
    flags = _sample_flags("samples", antithetic, qmc)
    _check_seed("samples", seed)
    if B == 0:
        return None, None, np.zeros(0, dtype=np.int64)
    n = _per_distribution_int("samples", "n", n, B)
    first = _per_distribution_int("samples", "first", first, B)
    streams = _checked_streams("samples", streams, B, "distribution")
    if streams is None:
        streams = np.arange(B, dtype=np.uint32)
    n_int, deg = _common_quadrature("samples", distrs)
    handles, r1, lam, sig = _batch_problem_args(distrs)
    a, b = _domain_arrays(distrs)
    total = int(n.sum())
    lib = _lib.lib()
    (out, u), kind = _output_arrays(device, [total, total if return_uniforms else None])
    _lib.check(lib.mlmc_density_sample_batch(B, C.cast(handles, C.c_void_p), _lib.ptr(r1), _lib.ptr(lam), _lib.ptr(sig), _lib.ptr(a),
                                             _lib.ptr(b), n_int, deg, int(seed), _lib.ptr(streams),
                                             _lib.ptr(first), _lib.ptr(n), flags,
                                             _lib.ptr(out), _lib.ptr(u), None, kind))
    return out, u, n


def sobol_table(seed, dims, scramble=True):
    """The table behind qmc=True (mlmc_sobol_table; host arithmetic, needs no device): for the dimensions `dims` (integers below
    1024) the 52 direction numbers [len(dims), 52] and the digital shifts [len(dims)] as uint64, scrambled under `seed`, or with
    scramble=False the raw Joe-Kuo numbers and zero shifts.  Point i of a dimension is the XOR of the direction numbers at the set
    bits of i ^ (i >> 1), XOR the shift; u = (2 m + 1) 2^-53."""
    _check_seed("sobol_table", seed)
    d = np.asarray(dims)
    if d.ndim != 1 or (d.size and (d.dtype.kind not in "iu" or np.any(d < 0) or np.any(d.astype(np.uint64) >= 2 ** 32))):
        raise ValueError("sobol_table: dims must be a 1-D array of integers in 0 .. 1023")
    d = np.ascontiguousarray(d.astype(np.uint32))
    dirs, shift = np.zeros((d.size, 52), dtype=np.uint64), np.zeros(d.size, dtype=np.uint64)
    _lib.check(_lib.load().mlmc_sobol_table(int(seed), 1 if scramble else 0, _lib.ptr(d), int(d.size), _lib.ptr(dirs), _lib.ptr(shift)))
    return dirs, shift


CorrelationFactorInfo = collections.namedtuple("CorrelationFactorInfo", "min_eig_in repaired max_change")


def correlation_factor(corr, min_eig=1e-10):
    """Lower-triangular factor F of a correlation matrix, F F^T = corr, for `joint_samples`; on the host in NumPy.  The matrix is
    symmetrised; it must be square and finite with a unit diagonal within 1e-8.  A multilevel covariance estimate is a telescoping
    sum and need not be positive definite: if the smallest eigenvalue is below `min_eig`, the eigenvalues are clipped to
    `min_eig`, the matrix is rebuilt and rescaled to a unit diagonal.  The rows of the Cholesky factor are renormalised to unit
    norm, so that every marginal of F z is a standard normal.
    :return: (factor [M, M], CorrelationFactorInfo(min_eig_in, repaired, max_change)): the smallest eigenvalue of the input,
        whether it was repaired, and the largest absolute change of an entry (F F^T against the symmetrised input)"""
    c = np.array(corr, dtype=np.float64)
    if c.ndim != 2 or c.shape[0] != c.shape[1] or c.shape[0] < 1:
        raise ValueError("correlation_factor: corr must be a square matrix, got shape {}".format(c.shape))
    if not np.all(np.isfinite(c)):
        raise ValueError("correlation_factor: corr must be finite")
    c = 0.5 * (c + c.T)
    if np.max(np.abs(np.diag(c) - 1.0)) > 1e-8:
        raise ValueError("correlation_factor: corr must have a unit diagonal (within 1e-8)")
    w, v = np.linalg.eigh(c)
    min_eig_in = float(w[0])
    repaired = bool(min_eig_in < min_eig)
    fixed = c
    if repaired:
        fixed = (v * np.maximum(w, min_eig)) @ v.T
        d = 1.0 / np.sqrt(np.diag(fixed))
        fixed = fixed * d[:, None] * d[None, :]
        fixed = 0.5 * (fixed + fixed.T)
    factor = np.linalg.cholesky(fixed)
    factor = np.ascontiguousarray(factor / np.sqrt(np.sum(factor * factor, axis=1))[:, None])
    return factor, CorrelationFactorInfo(min_eig_in, repaired, float(np.max(np.abs(factor @ factor.T - c))))


# the largest degrees of freedom of the mixing variable of a conditional t law, nu + p (include/mlmc_hip.h)
MAX_DOF_MIX = 192.0


def _check_dof(what, dof):
    """None for the Gaussian copula (dof None or +inf), else nu as a float in [1, 64]"""
    if dof is None:
        return None
    try:
        nu = float(dof)
    except (TypeError, ValueError):
        nu = np.nan
    if isinstance(dof, (bool, np.bool_)) or not (nu == np.inf or 1.0 <= nu <= 64.0):
        raise ValueError("{}: dof must lie in [1, 64] (None or inf: the Gaussian copula), got {!r}".format(what, dof))
    return None if nu == np.inf else nu


def _check_dof_mix(what, dof_mix):
    """the degrees of freedom of a conditional law's mixing variable, nu + p, as a float in [1, 192]"""
    try:
        nu = float(dof_mix)
    except (TypeError, ValueError):
        nu = np.nan
    if isinstance(dof_mix, (bool, np.bool_)) or not 1.0 <= nu <= MAX_DOF_MIX:
        raise ValueError("{}: dof_mix must lie in [1, {:g}], got {!r}".format(what, MAX_DOF_MIX, dof_mix))
    return nu


def _t_elementwise(what, entry, x, dof, device, mix=False):
    """one of the elementwise entries of the t copula on a NumPy array or a float64 device tensor of any shape; mix: dof is the
    dof_mix of `conditional_mixing_scale`"""
    nu = _check_dof_mix(what, dof) if mix else _check_dof(what, dof)
    if nu is None:
        raise ValueError(what + ": dof must be finite, in [1, 64]")
    if hasattr(x, "data_ptr"):
        import torch
        if not x.is_cuda or str(x.dtype) != "torch.float64":
            raise ValueError(what + ": the argument must be a NumPy array or a float64 device tensor")
        x = x.contiguous()
        out = torch.empty_like(x)
        torch.cuda.current_stream(x.device).synchronize()           # the library reads and writes on its own stream
        _lib.check(getattr(_lib.lib(), entry)(nu, int(x.numel()), _lib.ptr(x), _lib.ptr(out), _lib.DEVICE))
        return out if device else out.cpu().numpy()
    shape = np.shape(x)
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    out = np.empty_like(x)
    _lib.check(getattr(_lib.lib(), entry)(nu, int(x.size), _lib.ptr(x), _lib.ptr(out), _lib.HOST))
    out = out.reshape(shape)
    if device:
        import torch
        return torch.from_numpy(out).to(torch.device("cuda", torch.cuda.current_device()))
    return out if out.ndim else float(out)


def student_t_cdf(y, dof, device=False):
    """The CDF of Student's t with `dof` degrees of freedom (a float in [1, 64]) on the device, elementwise
    (mlmc_student_t_cdf): the function that the t copula of `joint_samples(dof=...)` maps with.  Relative accuracy in the lower
    tail; cdf(y) == 1 - cdf(-y) bit for bit for y > 0; 0 / 1 at -inf / +inf, NaN for NaN.
    :param y: a NumPy array or a float64 torch device tensor of any shape
    :param device: return a float64 torch device tensor"""
    return _t_elementwise("student_t_cdf", "mlmc_student_t_cdf", y, dof, device)


def chi2_mixing_scale(p, dof, device=False):
    """s = sqrt(dof / g) with g the p-quantile of the chi-square law with `dof` degrees of freedom (a float in [1, 64]) on the
    device, elementwise (mlmc_chi2_mixing_scale): a standard normal times s, p uniform, is a Student-t variate.  NaN for p
    outside (0, 1).
    :param p: a NumPy array or a float64 torch device tensor of any shape
    :param device: return a float64 torch device tensor"""
    return _t_elementwise("chi2_mixing_scale", "mlmc_chi2_mixing_scale", p, dof, device)


def conditional_mixing_scale(p, dof_mix, device=False):
    """`chi2_mixing_scale` for the mixing variable of `conditional_samples(dof=...)`, whose degrees of freedom dof + p may reach
    192 (mlmc_chi2_conditional_scale): dof_mix is a float in [1, 192]; up to 64 the values are those of `chi2_mixing_scale` bit
    for bit.
    :param p: a NumPy array or a float64 torch device tensor of any shape
    :param device: return a float64 torch device tensor"""
    return _t_elementwise("conditional_mixing_scale", "mlmc_chi2_conditional_scale", p, dof_mix, device, mix=True)


def _check_conditional_dof(what, dof, p):
    """the degrees of freedom nu + p of a t law conditioned on p components must stay within what the mixing scale is tested for"""
    if dof is not None and dof + p > MAX_DOF_MIX:
        raise ValueError("{}: dof + the number of given components = {:g} + {} exceeds {:g}, the largest degrees of freedom of the "
                         "conditional mixing variable".format(what, dof, p, MAX_DOF_MIX))


def _mixing_stream(what, dof, mix_stream, streams, K):
    """the stream of the mixing variable of a t copula, checked against the streams of the latent normals (None: stream k = k,
    and then K is the default)"""
    if dof is None:
        if mix_stream is not None:
            raise ValueError(what + ": mix_stream needs dof (the Gaussian copula has no mixing variable)")
        return None
    if mix_stream is None:
        if streams is not None:
            raise ValueError(what + ": with explicit streams, mix_stream must be given too")
        return K
    if isinstance(mix_stream, (bool, np.bool_)) or int(mix_stream) != mix_stream or not 0 <= int(mix_stream) < 2 ** 32:
        raise ValueError(what + ": mix_stream must be an integer in 0 .. 2^32 - 1")
    used = np.arange(K) if streams is None else np.asarray(streams)
    if np.any(used.astype(np.uint64) == np.uint64(int(mix_stream))):
        raise ValueError("{}: mix_stream {} is the stream of a latent normal".format(what, int(mix_stream)))
    return int(mix_stream)


def joint_samples(distrs, n, seed, corr=None, factor=None, streams=None, first=0, antithetic=False, device=False,
                  return_uniforms=False, return_normals=False, qmc=False, dof=None, mix_stream=None, return_mixing=False):
    """Seeded JOINT draws from many distributions through ONE device call (mlmc_density_sample_joint_batch): a Gaussian copula
    over the marginals.  With K latent standard normals z and a factor F [M, K] of the correlation matrix of the normal scores,
        x[m, j] = Q_m(u[m, j]),   u = clamp(Phi(F z)),
    Q_m of `quantiles` (bit for bit its value at p = u).  Latent normal k of draw j is Phi^-1 of the uniform j of stream streams[k]
    under `seed` that `samples` uses (include/mlmc_hip.h), so a draw depends on (seed, streams, j, antithetic, row m of F,
    distribution m, quadrature) alone: not on n, on first, on the other rows or on the batch.  With F = I the draws equal those of
    `samples` with the same seed and streams up to the rounding of Phi(Phi^-1(.)): give the two different seeds or streams where
    they must be independent of each other.
    :param n: draws per distribution (one integer); draw indices first .. first + n - 1
    :param seed: required, 0 <= seed < 2^64; there is no global generator
    :param corr: correlation matrix [M, M] of the normal scores; goes through `correlation_factor`
    :param factor: or the factor itself, [M, K] with rows of unit norm: K = M lower triangular, K < M a low-rank factor model,
        ones [M, 1] comonotone draws.  Exactly one of corr / factor must be given
    :param streams: one uint32 stream per latent normal; default: stream k = k
    :param antithetic: draws 2k and 2k + 1 come from z and -z
    :param qmc: randomised quasi-Monte Carlo (MLMC_SAMPLE_SOBOL): the uniform behind latent normal k is coordinate streams[k] of point j of the scrambled Sobol'
        sequence of include/mlmc_hip.h instead of the Philox uniform.  The streams are then DIMENSIONS and must be below 1024; n
        should be a power of two and `first` a multiple of it, since the points are balanced over blocks aligned to powers of two
        (any first and n are allowed).  For an error bar repeat with R seeds: the seeds give independent scrambles, and the sample
        standard deviation of the R means estimates the error of their mean.  Not together with antithetic
    :param device: return float64 torch device tensors
    :param dof: None or np.inf: the Gaussian copula above, bit for bit what it has always been.  A float in [1, 64]: a STUDENT-T
        copula with that many degrees of freedom (mlmc_density_sample_joint_t_batch), which has tail dependence:
            u = clamp(T_dof(s F z)),   s = sqrt(dof / chi2_dof) = chi2_mixing_scale(p0, dof),
        one mixing uniform p0 per draw (with antithetic one per pair, so that the pair negates y exactly), T_dof of
        `student_t_cdf`.  F is a factor of the copula's correlation matrix: for a t copula the correlation of the normal scores is
        NOT that matrix; `Estimate.estimate_quadrant_correlation` estimates it consistently.  Box probabilities and
        event scenarios under the same copula: `joint_probabilities(dof=...)`, `event_samples(dof=...)`; conditional draws,
        quantiles and CDFs: `conditional_samples(dof=...)`, `conditional_quantiles(dof=...)`, `conditional_cdfs(dof=...)`;
        conditional probabilities, event scenarios and aggregates: `conditional_probabilities(dof=...)`,
        `conditional_event_samples(dof=...)`, `conditional_aggregates(dof=...)`
    :param mix_stream: the uint32 stream (qmc: the dimension, below 1024) of the mixing uniform; default K when `streams` is
        defaulted; with explicit `streams` it must be given and differ from all of them
    :param return_uniforms, return_normals, return_mixing: also return u [M, n], z [K, n] and / or s [n] (dof only), in this order
    :return: draws [M, n]; every distribution must use the same quadrature"""
    distrs = list(distrs)
    M = len(distrs)
    flags = _sample_flags("joint_samples", antithetic, qmc)
    _check_seed("joint_samples", seed)
    dof = _check_dof("joint_samples", dof)
    if return_mixing and dof is None:
        raise ValueError("joint_samples: return_mixing needs dof (the Gaussian copula has no mixing variable)")
    if (corr is None) == (factor is None):
        raise ValueError("joint_samples: exactly one of corr and factor must be given")
    if M == 0:
        raise ValueError("joint_samples: no distributions")
    n = int(_per_distribution_int("joint_samples", "n", n, 1)[0])
    first = int(_per_distribution_int("joint_samples", "first", first, 1)[0])
    if corr is not None:
        factor = correlation_factor(corr)[0]
    factor = np.ascontiguousarray(factor, dtype=np.float64)
    if factor.ndim != 2 or factor.shape[0] != M or factor.shape[1] < 1:
        raise ValueError("joint_samples: the factor must be [M, K] with M = {} distributions, got shape {}".format(M, factor.shape))
    K = factor.shape[1]
    streams = _checked_streams("joint_samples", streams, K, "latent normal")
    mix_stream = _mixing_stream("joint_samples", dof, mix_stream, streams, K)
    n_int, deg = _common_quadrature("joint_samples", distrs)
    handles, r1, lam, sig = _batch_problem_args(distrs)
    a, b = _domain_arrays(distrs)
    (out, u, z, s), kind = _output_arrays(device, [(M, n), (M, n) if return_uniforms else None, (K, n) if return_normals else None,
                                                   (n,) if return_mixing else None])
    if dof is None:
        _lib.check(_lib.lib().mlmc_density_sample_joint_batch(
            M, C.cast(handles, C.c_void_p), _lib.ptr(r1), _lib.ptr(lam), _lib.ptr(sig), _lib.ptr(a), _lib.ptr(b), n_int, deg, K,
            _lib.ptr(factor), int(seed), _lib.ptr(streams), first, n, flags, _lib.ptr(out), _lib.ptr(u), _lib.ptr(z), None, kind))
    else:
        _lib.check(_lib.lib().mlmc_density_sample_joint_t_batch(
            M, C.cast(handles, C.c_void_p), _lib.ptr(r1), _lib.ptr(lam), _lib.ptr(sig), _lib.ptr(a), _lib.ptr(b), n_int, deg, K,
            _lib.ptr(factor), dof, int(seed), _lib.ptr(streams), mix_stream, first, n, flags, _lib.ptr(out), _lib.ptr(u), _lib.ptr(z),
            _lib.ptr(s), None, kind))
    extra = tuple(v for v, want in ((u, return_uniforms), (z, return_normals), (s, return_mixing)) if want)
    return (out,) + extra if extra else out


ConditionalFactorInfo = collections.namedtuple("ConditionalFactorInfo", "unobserved s min_eig_in repaired")


def conditional_factor(corr, observed, min_eig=1e-10, return_observed=False):
    """What conditioning a Gaussian copula on the components `observed` needs, on the host in NumPy.  With C' = F F^T of
    `correlation_factor(corr, min_eig)` (repaired, unit diagonal), O = the observed components ascending, U the others ascending
    and L = cholesky(C'[P, P]) for P = O ++ U in blocks L_OO, L_UO, L_UU, the scores of U given the scores z_O of O are normal with
        mean  W z_O,  W = L_UO L_OO^-1 [q, p] (a triangular solve),   and factor  F_c = L_UU [q, q] (lower triangular),
    so their covariance F_c F_c^T (the Schur complement C'_UU - C'_UO C'_OO^-1 C'_OU) does not depend on z_O.  Row m of F_c has
    norm s_m in (0, 1], the conditional standard deviation of score m, and |L_UO[m]|^2 + s_m^2 = 1.
    :param observed: distinct component indices in any order; may be empty: then W is [M, 0] and F_c the factor of
        `correlation_factor` itself
    :param return_observed: also return L_OO [p, p], the Cholesky factor of C'[O, O]: what the Student-t copula needs in addition,
        since its conditional scale depends on d = |L_OO^-1 y_O|^2 (`conditional_samples(dof=...)`)
    :return: (W [q, p], F_c [q, q], ConditionalFactorInfo(unobserved [q], s [q], min_eig_in, repaired)), the last two those of
        `correlation_factor`; with return_observed a fourth item L_OO"""
    factor, info = correlation_factor(corr, min_eig)
    M = factor.shape[0]
    observed = list(observed)
    if any(isinstance(o, (bool, np.bool_)) or not isinstance(o, (int, np.integer)) for o in observed):
        raise ValueError("conditional_factor: observed must hold component indices, got {!r}".format(observed))
    obs = np.array(observed, dtype=np.int64).reshape(-1)
    if np.any(obs < 0) or np.any(obs >= M):
        raise ValueError("conditional_factor: observed component out of range 0 .. {}: {}".format(M - 1, obs.tolist()))
    if np.unique(obs).size != obs.size:
        raise ValueError("conditional_factor: observed components must be distinct: {}".format(obs.tolist()))
    obs = np.sort(obs)
    p = obs.size
    if p == M:
        raise ValueError("conditional_factor: every component is observed, nothing is left to condition")
    unobs = np.setdiff1d(np.arange(M, dtype=np.int64), obs)
    l_oo = np.zeros((0, 0))
    if p == 0:
        w, fc = np.zeros((M, 0)), factor
    else:
        perm = np.concatenate([obs, unobs])
        c = factor @ factor.T
        c = 0.5 * (c + c.T)
        low = np.linalg.cholesky(c[np.ix_(perm, perm)])
        w = scipy.linalg.solve_triangular(low[:p, :p], low[p:, :p].T, lower=True, trans="T").T
        fc = np.ascontiguousarray(low[p:, p:])
        l_oo = np.ascontiguousarray(low[:p, :p])
    s = np.sqrt(np.sum(fc * fc, axis=1))
    out = (np.ascontiguousarray(w), fc, ConditionalFactorInfo(unobs, s, info.min_eig_in, info.repaired))
    return out + (l_oo,) if return_observed else out


def _parse_given(what, given, M):
    """(observed [p] ascending, values [p, B], every value a scalar?) of a mapping component -> scalar or array [B]; scalars next to
    arrays stand for the same value in every set"""
    if not hasattr(given, "items"):
        raise ValueError(what + ": given must map component indices to values")
    keys, vals = [], []
    for k, v in given.items():
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
            raise ValueError(what + ": a key of given must be a component index, got {!r}".format(k))
        if not 0 <= int(k) < M:
            raise ValueError(what + ": given names component {}, there are components 0 .. {}".format(int(k), M - 1))
        v = np.asarray(v, dtype=np.float64)
        if v.ndim > 1:
            raise ValueError(what + ": the value of component {} must be a scalar or a 1-D array, got shape {}".format(int(k), v.shape))
        keys.append(int(k))
        vals.append(v)
    if len(set(keys)) != len(keys):
        raise ValueError(what + ": given names a component twice")
    if len(keys) == M:
        raise ValueError(what + ": every component is given, nothing is left to condition")
    sizes = {v.size for v in vals if v.ndim == 1}
    if len(sizes) > 1:
        raise ValueError(what + ": the arrays of given must share one length, got {}".format(sorted(sizes)))
    scalar = not sizes
    B = 1 if scalar else sizes.pop()
    if B < 1:
        raise ValueError(what + ": the arrays of given are empty")
    order = np.argsort(keys) if keys else []
    observed = np.array([keys[i] for i in order], dtype=np.int64)
    values = np.empty((len(keys), B))
    for row, i in enumerate(order):
        values[row] = vals[i]
    return observed, values, scalar


def _conditional_t_scale(y_obs, l_oo, dof):
    """r [B] = sqrt((nu + d) / (nu + p)), d = |L_OO^-1 y_O|^2, for the t scores y_O [p, B] of the given values: the factor by which a
    Student-t copula widens (d > p) or narrows the conditional law of the other components; touches no device"""
    y_obs = np.asarray(y_obs, dtype=np.float64)
    p = y_obs.shape[0]
    if p == 0:
        return np.ones(y_obs.shape[1])
    v = scipy.linalg.solve_triangular(np.asarray(l_oo, dtype=np.float64), y_obs, lower=True)
    return np.sqrt((dof + np.sum(v * v, axis=0)) / (dof + p))


def _conditioning(what, distrs, given, corr, cond, dof=None):
    """what the conditional entries share: (observed [p], values [p, B], scalar?, u_O [p, B], (W, F_c, info), mu [B, q], r [B]):
    the scores of the given values through ONE `normal_scores` call and the conditional means W z_O on the host.  With dof (a
    Student-t copula) the scores are the t scores y_O, `cond` is the 4-tuple of conditional_factor(return_observed=True) and r
    its conditional scale (`_conditional_t_scale`); without it r is ones"""
    M = len(distrs)
    if M == 0:
        raise ValueError(what + ": no distributions")
    observed, values, scalar = _parse_given(what, given, M)
    _check_conditional_dof(what, dof, observed.size)
    if (corr is None) == (cond is None):
        raise ValueError(what + ": exactly one of corr and the result of conditional_factor must be given")
    if cond is None:
        cond = conditional_factor(corr, observed, return_observed=dof is not None)
    if dof is not None and len(cond) != 4:
        raise ValueError(what + ": with dof, factor_info must be the 4-tuple of conditional_factor(..., return_observed=True): the "
                         "conditional scale of a t copula needs L_OO")
    l_oo = np.asarray(cond[3], dtype=np.float64) if dof is not None else None
    w, fc, info = cond[:3]
    w, fc = np.asarray(w, dtype=np.float64), np.ascontiguousarray(fc, dtype=np.float64)
    p, q, B = observed.size, M - observed.size, values.shape[1]
    if w.shape != (q, p) or fc.ndim != 2 or fc.shape[0] != q or fc.shape[1] < 1 \
            or not np.array_equal(np.asarray(info.unobserved), np.setdiff1d(np.arange(M), observed)):
        raise ValueError(what + ": the conditional factor does not belong to the components of given")
    if l_oo is not None and l_oo.shape != (p, p):
        raise ValueError(what + ": the conditional factor does not belong to the components of given")
    if p == 0:
        return observed, values, scalar, np.empty((0, B)), (w, fc, info), np.zeros((B, q)), np.ones(B)
    z, u = normal_scores([distrs[o] for o in observed], values, return_uniforms=True)
    bad = np.argwhere(~np.isfinite(z))
    if bad.size:
        raise ValueError(what + ": the given value {!r} of component {} (set {}) is NaN or outside the open domain of its "
                         "distribution".format(float(values[bad[0, 0], bad[0, 1]]), int(observed[bad[0, 0]]), int(bad[0, 1])))
    if dof is None:
        return observed, values, scalar, u, (w, fc, info), np.ascontiguousarray((w @ z).T), np.ones(B)
    y = t_scores(z, dof)
    return observed, values, scalar, u, (w, fc, info), np.ascontiguousarray((w @ y).T), _conditional_t_scale(y, l_oo, dof)


def conditional_samples(distrs, n, seed, given, corr=None, factor_info=None, streams=None, first=0, antithetic=False, device=False,
                        return_uniforms=False, qmc=False, dof=None, mix_stream=None, return_mixing=False):
    """Seeded joint draws of the components that are NOT in `given`, conditional on the given values of the others, under the
    Gaussian copula of `joint_samples`; B sets of given values through ONE device call (mlmc_density_sample_conditional_batch).
    The given values go to normal scores z_O (one `normal_scores` call); with (W, F_c) of `conditional_factor` the scores of the
    other components are W z_O + F_c z, z the latent normals of `joint_samples` (same seed, streams, first, antithetic), and
        x[b, m, j] = Q_m(clamp(Phi(mu[b, m] + (F_c z)[m, j]))),   mu[b] = W z_O[b].
    The tables of the marginals, the normals and their launch are made once for all sets; no value depends on B or on the
    position of a set.
    :param given: mapping component index -> scalar, or -> array [B] (all arrays share B; a scalar next to arrays holds in every
        set).  A value that is NaN or outside the open domain of its distribution is an error that names component and set.  An
        empty mapping gives the draws of `joint_samples` bit for bit
    :param corr: correlation matrix [M, M] of the normal scores of ALL components
    :param factor_info: or the tuple `conditional_factor(corr, observed)` returned.  Exactly one of the two must be given
    :param streams: one uint32 stream per latent normal (there are q = M - len(given)); default: stream k = k
    :param qmc: randomised quasi-Monte Carlo (MLMC_SAMPLE_SOBOL): the uniform behind latent normal k is coordinate streams[k] of point j of the scrambled Sobol'
        sequence of include/mlmc_hip.h instead of the Philox uniform.  The streams are then DIMENSIONS and must be below 1024; n
        should be a power of two and `first` a multiple of it, since the points are balanced over blocks aligned to powers of two
        (any first and n are allowed).  For an error bar repeat with R seeds: the seeds give independent scrambles, and the sample
        standard deviation of the R means estimates the error of their mean.  Not together with antithetic
    :param return_uniforms: also return u shaped like the draws; rows of given components hold Fhat_o(x_o)
    :param dof: None or np.inf: the Gaussian copula above, bit for bit what it has always been.  A float in [1, 64]: the STUDENT-T
        copula of `joint_samples(dof=...)` (mlmc_density_sample_conditional_t_batch).  Given the t scores y_O = t_scores(z_O, dof)
        of the p given values, the t scores of the others are multivariate t with dof + p degrees of freedom, location W y_O and
        scale matrix r^2 F_c F_c^T, r^2 = (dof + d) / (dof + p), d = |L_OO^-1 y_O|^2:
            x[b, m, j] = Q_m(clamp(T_dof(mu[b, m] + r_b s_c[j] (F_c z)[m, j]))),   s_c = conditional_mixing_scale(p0, dof + p),
        so an extreme given value WIDENS the law of the others (under the Gaussian copula the spread never depends on what was
        observed).  dof + p must not exceed 192.  W, F_c and L_OO come from the same repaired matrix:
        `factor_info` must then be the 4-tuple of conditional_factor(..., return_observed=True).  An empty `given` gives the draws
        of `joint_samples(dof=...)` bit for bit
    :param mix_stream: the stream (qmc: the dimension, below 1024) of the mixing uniform, as in `joint_samples`: default K when
        `streams` is defaulted, required and different from all of them otherwise
    :param return_mixing: also return the mixing scales s_c [n] (dof only), after the uniforms
    :return: draws [M, n] when every given value is a scalar, [B, M, n] otherwise: rows of the other components hold the draws, rows
        of given components the given values exactly; float64 torch device tensors with device=True"""
    what = "conditional_samples"
    distrs = list(distrs)
    M = len(distrs)
    flags = _sample_flags(what, antithetic, qmc)
    _check_seed(what, seed)
    dof = _check_dof(what, dof)
    if return_mixing and dof is None:
        raise ValueError(what + ": return_mixing needs dof (the Gaussian copula has no mixing variable)")
    if dof is None:
        _mixing_stream(what, dof, mix_stream, None, 0)
    n = int(_per_distribution_int(what, "n", n, 1)[0])
    first = int(_per_distribution_int(what, "first", first, 1)[0])
    observed = _parse_given(what, given, M)[0]  # its errors come before anything touches the device; one of them is M = 0
    if dof is not None:                         # and so do those of the t copula: the factor is host work
        _check_conditional_dof(what, dof, observed.size)
        if (corr is None) == (factor_info is None):
            raise ValueError(what + ": exactly one of corr and the result of conditional_factor must be given")
        if factor_info is None:
            factor_info, corr = conditional_factor(corr, observed, return_observed=True), None
        if len(factor_info) != 4:
            raise ValueError(what + ": with dof, factor_info must be the 4-tuple of conditional_factor(..., return_observed=True): "
                             "the conditional scale of a t copula needs L_OO")
        if np.ndim(factor_info[1]) != 2 or np.shape(factor_info[1])[1] < 1:
            raise ValueError(what + ": the conditional factor does not belong to the components of given")
        K = np.shape(factor_info[1])[1]
        mix_stream = _mixing_stream(what, dof, mix_stream, _checked_streams(what, streams, K, "latent normal"), K)
        if qmc and mix_stream >= 1024:
            raise ValueError(what + ": with qmc mix_stream is a Sobol' dimension and must be below 1024")
    n_int, deg = _common_quadrature(what, distrs)
    observed, values, scalar, u_obs, (_, fc, info), mu, r = _conditioning(what, distrs, given, corr, factor_info, dof)
    unobs = np.ascontiguousarray(info.unobserved, dtype=np.int32)
    q, K, B = unobs.size, fc.shape[1], values.shape[1]
    streams = _checked_streams(what, streams, K, "latent normal")
    free = [distrs[m] for m in unobs]
    handles, r1, lam, sig = _batch_problem_args(free)
    a, b = _domain_arrays(free)
    # the arrays are not those of _output_arrays: the rows of the given components are filled in before the synchronise
    if device:
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        out = torch.empty((B, M, n), dtype=torch.float64, device=dev)
        u = torch.empty((B, M, n), dtype=torch.float64, device=dev) if return_uniforms else None
        s = torch.empty((n,), dtype=torch.float64, device=dev) if return_mixing else None
        if observed.size:
            out[:, observed.tolist(), :] = torch.from_numpy(np.ascontiguousarray(values.T)).to(dev)[:, :, None]
            if u is not None:
                u[:, observed.tolist(), :] = torch.from_numpy(np.ascontiguousarray(u_obs.T)).to(dev)[:, :, None]
        torch.cuda.current_stream(dev).synchronize()         # the library writes the other rows on its own stream
        kind = _lib.DEVICE
    else:
        out = np.empty((B, M, n))
        u = np.empty((B, M, n)) if return_uniforms else None
        s = np.empty(n) if return_mixing else None
        out[:, observed, :] = values.T[:, :, None]
        if u is not None:
            u[:, observed, :] = u_obs.T[:, :, None]
        kind = _lib.HOST
    if dof is None:
        _lib.check(_lib.lib().mlmc_density_sample_conditional_batch(
            q, C.cast(handles, C.c_void_p), _lib.ptr(r1), _lib.ptr(lam), _lib.ptr(sig), _lib.ptr(a), _lib.ptr(b),
            n_int, deg, K, _lib.ptr(fc), int(seed), _lib.ptr(streams), first, n,
            flags, B, _lib.ptr(mu) if observed.size else None, _lib.ptr(unobs), M, _lib.ptr(out),
            _lib.ptr(u), None, None, kind))
    else:
        r = np.ascontiguousarray(r, dtype=np.float64)
        _lib.check(_lib.lib().mlmc_density_sample_conditional_t_batch(
            q, C.cast(handles, C.c_void_p), _lib.ptr(r1), _lib.ptr(lam), _lib.ptr(sig), _lib.ptr(a), _lib.ptr(b),
            n_int, deg, K, _lib.ptr(fc), dof, dof + observed.size, int(seed), _lib.ptr(streams), mix_stream, first, n,
            flags, B, _lib.ptr(mu) if observed.size else None, _lib.ptr(r) if observed.size else None, _lib.ptr(unobs), M,
            _lib.ptr(out), _lib.ptr(u), None, _lib.ptr(s), None, kind))
    if scalar:
        out, u = out[0], (None if u is None else u[0])
    extra = tuple(v for v, want in ((u, return_uniforms), (s, return_mixing)) if want)
    return (out,) + extra if extra else out


def _conditional_law(what, distrs, given, corr, dof=None):
    """(the distributions that are not given, mu [B, q], s [q], every given value a scalar?, dof or None, r [B], the number of
    given components) of `conditional_quantiles` / `_cdfs`"""
    distrs = list(distrs)
    dof = _check_dof(what, dof)
    if dof is not None:                          # before anything touches the device
        _check_conditional_dof(what, dof, _parse_given(what, given, len(distrs))[0].size)
    observed, _, scalar, _, (_, _, info), mu, r = _conditioning(what, distrs, given, corr, None, dof)
    return [distrs[m] for m in info.unobserved], mu, np.asarray(info.s), scalar, dof, r, observed.size


def _t_cdf_lower_tail(y, dof):
    """T_dof(y) through the lower tail on either side (SciPy's stdtr), as `t_scores` inverts it"""
    from scipy.special import stdtr
    y = np.asarray(y, dtype=np.float64)
    low = stdtr(float(dof), -np.abs(y))
    return np.where(y > 0, 1.0 - low, low)


def _t_quantile_lower_tail(p, dof):
    """T_dof^-1(p) through the lower tail on either side (SciPy's stdtrit): -inf / +inf at 0 / 1, NaN for what is no probability"""
    from scipy.special import stdtrit
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        upper = p > 0.5
        t = stdtrit(float(dof), np.where(upper, 1.0 - p, p))
        t = np.where(upper, -t, t)
        t = np.where(p == 0.0, -np.inf, np.where(p == 1.0, np.inf, t))
    return np.where((p >= 0.0) & (p <= 1.0), t, np.nan)


def _t_conditional_quantile_map(p, mu, scale, dof, dof_c):
    """p' = T_dof(mu + scale T_dofc^-1(p)): where the conditional quantile at p of a score that is t with dof_c degrees of freedom,
    location mu and the given scale lies under its marginal t law with dof; host only, broadcasting"""
    with np.errstate(invalid="ignore"):
        return _t_cdf_lower_tail(mu + scale * _t_quantile_lower_tail(p, dof_c), dof)


def _t_conditional_cdf_map(f, mu, scale, dof, dof_c):
    """T_dofc((T_dof^-1(f) - mu) / scale), the inverse of `_t_conditional_quantile_map`; host only, broadcasting"""
    with np.errstate(invalid="ignore"):
        return _t_cdf_lower_tail((_t_quantile_lower_tail(f, dof) - mu) / scale, dof_c)


def conditional_quantiles(distrs, probs, given, corr, dof=None):
    """Quantiles of every component that is not in `given`, conditional on the given values of the others, under the Gaussian
    copula: given z_O the score of component m is N(mu_m, s_m^2) (`conditional_factor`), so its conditional quantile at p is
        Q_m(p'),   p' = Phi(mu_m + s_m Phi^-1(p)),
    mapped on the host (SciPy's ndtri / ndtr) and inverted by ONE `quantiles` call for all sets, components and probabilities.
    p = 0 and p = 1 give the end points of the domain exactly, a NaN or out-of-range p gives NaN.
    :param probs: [P] probabilities, the same for every component and set
    :param given, corr: as in `conditional_samples`
    :param dof: None or np.inf: the Gaussian copula.  A float in [1, 64]: the Student-t copula of `conditional_samples(dof=...)`:
        the t score of component m given y_O is univariate t with dof + p degrees of freedom, location mu_m and scale r_b s_m, so
            p' = T_dof(mu_m + r_b s_m T_{dof + p}^-1(p))
        (SciPy's stdtrit / stdtr through the lower tail on either side, as `t_scores`)
    :return: [q, P] when every given value is a scalar, [B, q, P] otherwise; row m = component info.unobserved[m]"""
    from scipy.special import ndtr, ndtri
    free, mu, s, scalar, dof, r, n_given = _conditional_law("conditional_quantiles", distrs, given, corr, dof)
    probs = np.atleast_1d(np.asarray(probs, dtype=np.float64)).reshape(-1)
    with np.errstate(invalid="ignore"):
        if dof is None:
            mapped = ndtr(mu[:, :, None] + s[None, :, None] * ndtri(probs)[None, None, :])         # [B, q, P]
        else:
            mapped = _t_conditional_quantile_map(probs[None, None, :], mu[:, :, None], r[:, None, None] * s[None, :, None], dof,
                                                 dof + n_given)
    q = quantiles(free, [np.ascontiguousarray(mapped[:, m, :]).reshape(-1) for m in range(len(free))])
    out = np.stack([np.asarray(r).reshape(mu.shape[0], probs.size) for r in q], axis=1)
    return out[0] if scalar else out


def conditional_cdfs(distrs, values, given, corr, dof=None):
    """Conditional CDFs of every component that is not in `given`, the inverse of `conditional_quantiles`:
        Phi((Phi^-1(clamp(Fhat_m(x))) - mu_m) / s_m),
    Fhat_m through ONE `cdfs_on_rule` call, the clamp to [2^-53, 1 - 2^-53] of `normal_scores`, the map on the host.
    :param values: an array that broadcasts to [B, q, P] ([P]: the same points for every component and set; the result of
        `conditional_quantiles` as it is)
    :param dof: None or np.inf: the Gaussian copula.  A float in [1, 64]: the Student-t copula of `conditional_quantiles(dof=...)`,
        T_{dof + p}((T_dof^-1(clamp(Fhat_m(x))) - mu_m) / (r_b s_m))
    :return: [q, P] when every given value is a scalar, [B, q, P] otherwise"""
    from scipy.special import ndtr, ndtri
    free, mu, s, scalar, dof, r, n_given = _conditional_law("conditional_cdfs", distrs, given, corr, dof)
    values = np.asarray(values, dtype=np.float64)
    B, q = mu.shape
    x = np.broadcast_to(values, (B, q) + values.shape[-1:]) if values.ndim else np.broadcast_to(values, (B, q, 1))
    f = cdfs_on_rule(free, [np.ascontiguousarray(x[:, m, :]).reshape(-1) for m in range(q)])
    f = np.stack([np.asarray(r).reshape(B, -1) for r in f], axis=1)
    f = np.minimum(np.maximum(f, 2.0 ** -53), 1.0 - 2.0 ** -53)
    if dof is None:
        out = ndtr((ndtri(f) - mu[:, :, None]) / s[None, :, None])
    else:
        out = _t_conditional_cdf_map(f, mu[:, :, None], r[:, None, None] * s[None, :, None], dof, dof + n_given)
    return out[0] if scalar else out


JointProbability = collections.namedtuple("JointProbability", "prob stderr replicates n seeds")


def _box_call_args(what, n, seeds, first):
    """(n, seeds [R] uint64, first) of a box-probability call, checked"""
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError(what + ": n must be a positive integer")
    if isinstance(first, (bool, np.bool_)) or not isinstance(first, (int, np.integer)) or first < 0:
        raise ValueError(what + ": first must be a non-negative integer")
    if int(first) + int(n) > 2 ** 52:
        raise ValueError(what + ": first + n must not exceed 2^52")
    try:
        seed_list = list(seeds)
    except TypeError:
        raise ValueError(what + ": seeds must be a sequence of integers in 0 .. 2^64 - 1") from None
    if not seed_list:
        raise ValueError(what + ": at least one seed is required")
    for s in seed_list:
        if isinstance(s, (bool, np.bool_)) or not isinstance(s, (int, np.integer)) or not 0 <= int(s) < 2 ** 64:
            raise ValueError(what + ": seeds must be integers in 0 .. 2^64 - 1, got {!r}".format(s))
    return int(n), np.array([int(s) for s in seed_list], dtype=np.uint64), int(first)


def _box_limits(what, lower, upper, M, name="M"):
    """lower and upper broadcast to one [B, M] pair; a NaN is an error that names box and component"""
    lo, hi = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    if lo.ndim > 2 or hi.ndim > 2:
        raise ValueError(what + ": lower and upper must broadcast to [B, {}]".format(name))
    try:
        shape = np.broadcast_shapes(lo.shape, hi.shape, (1, M))
    except ValueError:
        raise ValueError(what + ": lower {} and upper {} do not broadcast to [B, {}] with {} = {}".format(
            lo.shape, hi.shape, name, name, M)) from None
    if shape[1] != M or shape[0] < 1:
        raise ValueError(what + ": lower {} and upper {} do not broadcast to [B, {}] with {} = {}".format(
            lo.shape, hi.shape, name, name, M))
    lo, hi = np.ascontiguousarray(np.broadcast_to(lo, shape)), np.ascontiguousarray(np.broadcast_to(hi, shape))
    bad = np.argwhere(np.isnan(lo) | np.isnan(hi))
    if bad.size:
        raise ValueError(what + ": a limit of box {}, component {} is NaN".format(int(bad[0, 0]), int(bad[0, 1])))
    return lo, hi


def _box_streams(what, streams, M, qmc):
    st = _checked_streams(what, streams, M - 1, "coordinate, {} of them".format(M - 1))
    if qmc and st is not None and np.any(st >= 1024):
        raise ValueError(what + ": with qmc the streams are Sobol' dimensions and must be below 1024")
    return st


def _box_problem(what, factor, lower, upper, shift, per_box=False):
    """(factor [M, M] lower triangular, lo [B, M], hi [B, M], shift [B, M] or None) of a call in score space, checked; with
    per_box a factor [B, M, M], one per box, is accepted too (one box of limits then pairs with every factor)"""
    f = np.array(factor, dtype=np.float64)
    if per_box and f.ndim == 3:
        return _box_problem_per_box(what, f, lower, upper, shift)
    if f.ndim != 2 or f.shape[0] != f.shape[1] or f.shape[0] < 1:
        raise ValueError(what + ": the factor must be a square matrix{}, got shape {}".format(
            " [M, M] or one per box [B, M, M]" if per_box else "", f.shape))
    M = f.shape[0]
    if M > _lib.BOX_PROB_MAX_M:
        raise ValueError(what + ": {} components exceed the cap of {}".format(M, _lib.BOX_PROB_MAX_M))
    f = np.ascontiguousarray(np.tril(f))
    diag = np.diag(f)
    bad = np.flatnonzero(~(np.isfinite(diag) & (diag > 0)))
    if bad.size:
        raise ValueError(what + ": the diagonal entry of factor row {} must be finite and positive, got {}".format(
            int(bad[0]), diag[bad[0]]))
    if not np.all(np.isfinite(f)):
        raise ValueError(what + ": factor row {} has an entry that is not finite".format(int(np.argwhere(~np.isfinite(f))[0, 0])))
    lo, hi = _box_limits(what, lower, upper, M)
    return (f,) + _box_shift(what, lo, hi, shift)


def _box_problem_per_box(what, f, lower, upper, shift):
    """`_box_problem` for one factor per box, f [B, M, M]: the same checks on every factor, the errors name the box"""
    if f.shape[1] != f.shape[2] or f.shape[0] < 1 or f.shape[1] < 1:
        raise ValueError(what + ": the factors must be [B, M, M] with B >= 1 and M >= 1, got shape {}".format(f.shape))
    B, M = f.shape[0], f.shape[1]
    if M > _lib.BOX_PROB_MAX_M:
        raise ValueError(what + ": {} components exceed the cap of {}".format(M, _lib.BOX_PROB_MAX_M))
    f = np.ascontiguousarray(np.tril(f))
    diag = np.diagonal(f, axis1=1, axis2=2)
    bad = np.argwhere(~(np.isfinite(diag) & (diag > 0)))
    if bad.size:
        raise ValueError(what + ": box {}: the diagonal entry of factor row {} must be finite and positive, got {}".format(
            int(bad[0, 0]), int(bad[0, 1]), diag[bad[0, 0], bad[0, 1]]))
    bad = np.argwhere(~np.isfinite(f))
    if bad.size:
        raise ValueError(what + ": box {}: factor row {} has an entry that is not finite".format(int(bad[0, 0]), int(bad[0, 1])))
    lo, hi = _box_limits(what, lower, upper, M)
    if lo.shape[0] == 1 and B > 1:
        lo, hi = np.repeat(lo, B, axis=0), np.repeat(hi, B, axis=0)
    if lo.shape[0] != B:
        raise ValueError(what + ": {} factors, one per box, but the limits hold {} boxes".format(B, lo.shape[0]))
    return (f,) + _box_shift(what, lo, hi, shift)


def _box_shift(what, lo, hi, shift):
    """(lo, hi, shift broadcast to [B, M] or None), the shift checked"""
    B, M = lo.shape
    if shift is not None:
        sh = np.asarray(shift, dtype=np.float64)
        try:
            sh = np.ascontiguousarray(np.broadcast_to(sh, (B, M)))
        except ValueError:
            raise ValueError(what + ": shift {} does not broadcast to [B, M] = {}".format(sh.shape, (B, M))) from None
        if not np.all(np.isfinite(sh)):
            raise ValueError(what + ": the shift must be finite")
        shift = sh
    return lo, hi, shift


def _box_t_streams(what, dof, shift, streams, mix_stream, count, qmc):
    """(chain streams uint32 [count], mixing stream) of a box call under the t copula, checked: by default the mixing variable takes
    stream 0, the lowest Sobol' dimension (Genz and Bretz's order), and chain coordinate i stream i + 1"""
    if shift is not None:
        raise ValueError(what + ": dof together with shift: this entry has no conditional law under the t copula (its mixing variable "
                         "has dof + p degrees of freedom); call conditional_box_probabilities / conditional_box_draws")
    if streams is None:
        streams = np.arange(1, count + 1, dtype=np.uint32)
        if mix_stream is None:
            return streams, 0
    mix_stream = _mixing_stream(what, dof, mix_stream, streams, count)
    if qmc and mix_stream >= 1024:
        raise ValueError(what + ": with qmc mix_stream is a Sobol' dimension and must be below 1024")
    return streams, mix_stream


def t_scores(z, dof):
    """The Student-t scores of normal scores z, on the host: y with T_dof(y) = Phi(z), through the lower tail on either side so
    that a far upper score keeps its relative accuracy: y = stdtrit(dof, ndtr(z)) for z <= 0 and -stdtrit(dof, ndtr(-z)) for z > 0
    (scipy.special).  Infinite scores are kept, 0 gives 0, NaN stays NaN; odd in z bit for bit."""
    from scipy.special import ndtr, stdtrit
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        y = np.where(z > 0, -1.0, 1.0) * stdtrit(float(dof), ndtr(-np.abs(z)))
    return np.where(np.isinf(z) | (z == 0), z, y)


def _check_mixing(what, mixing, dof, shift=None, given=None):
    """True for mixing="conditioned" (the tl entries), checked; touches no device"""
    if mixing not in ("plain", "conditioned"):
        raise ValueError(what + ': mixing must be "plain" or "conditioned", got {!r}'.format(mixing))
    if mixing == "plain":
        return False
    if dof is None:
        raise ValueError(what + ': mixing="conditioned" needs dof (the Gaussian copula has no mixing variable)')
    if shift is not None:
        raise ValueError(what + ': mixing="conditioned" together with shift: the conditioned lead exists for the unconditional t law only')
    if given is not None:
        raise ValueError(what + ': mixing="conditioned" together with given: the conditional family keeps plain mixing (its mixing '
                         "variable would have dof + p + 1 degrees of freedom, outside the tested range of the t functions)")
    return True


def copula_box_probabilities(factor, lower, upper, n, seeds, shift=None, streams=None, first=0, qmc=True, return_integrand=False,
                             device=False, dof=None, mix_stream=None, return_mixing=False, mixing="plain", return_lead=False):
    """P(lower < Y < upper) for Y = shift + F z, z standard normal, for B boxes and R seeds through ONE device call
    (mlmc_copula_box_prob_batch): Genz's separation of variables, which conditions through the lower-triangular factor with one
    Phi^-1 and two Phi per component, so that the integrand is a smooth function on the unit cube.  Everything is in SCORE space
    (`joint_probabilities` maps limits in the components' own units).  On scrambled Sobol' points (qmc=True) the error falls
    like 1 / n and is relative: a probability of 1e-8 is resolved as well as one of 0.1, which counting scenarios of
    `joint_samples` cannot do.  Each seed gives one independent estimate; `prob` is their mean and `stderr` the sample standard
    deviation of the R means over sqrt(R) (NaN for one seed).  A replicate depends on (factor, box, seed, streams, first, n, qmc)
    alone and is bitwise repeatable.
    :param factor: [M, M] lower triangular with a positive diagonal (the upper part is ignored); rows need not have unit norm, so
        F_c of `conditional_factor` is accepted.  M <= 128.  Or [B, M, M]: ONE FACTOR PER BOX, still one device call
        (mlmc_copula_box_prob_pf_batch and its t twins; every `dof` and `mixing`): box b is integrated through factor[b], as
        `box_order` and the bootstrap of a correlation matrix need it.  One box of limits pairs with every factor.  A box gives bit
        for bit what a call with its factor alone gives, and B copies of one factor give what [M, M] gives
    :param lower, upper: broadcast to [B, M], +-inf allowed; a box that is empty in some component has probability exactly 0
    :param n: points per seed, indices first .. first + n - 1; with qmc a power of two with `first` a multiple of it
    :param seeds: R integers in 0 .. 2^64 - 1
    :param shift: None or the mean of the scores, broadcast to [B, M]
    :param streams: one stream (qmc: Sobol' dimension below 1024) per coordinate, M - 1 of them; default: i
    :param qmc: scrambled Sobol' points (MLMC_SAMPLE_SOBOL); False: Philox uniforms
    :param return_integrand: also return the integrand [R, B, n] (a float64 torch device tensor with device=True)
    :param dof: None or np.inf: the Gaussian law above, bit for bit what it has always been.  A float in [1, 64]: Y = s F z is a
        multivariate STUDENT-T vector with that many degrees of freedom (mlmc_copula_box_prob_t_batch), s = chi2_mixing_scale(p0,
        dof) one mixing scale per point: P(lower < Y < upper) = E_s[P(lower / s < F z < upper / s)] (Genz and Bretz), one more
        coordinate per point, every limit divided by s, the rest the Gaussian chain.  The limits are T SCORES (`t_scores`).  Not
        together with `shift`: a conditional law of the t copula is `conditional_box_probabilities`
    :param mix_stream: the stream (qmc: the dimension, below 1024) of the mixing uniform.  Default 0, and chain coordinate i then
        takes stream i + 1; with explicit `streams` it must be given and differ from all of them
    :param return_mixing: also return the mixing scales s [R, n] (dof only), after the integrand
    :param mixing: "plain" (default): the mixing scale is sampled as it is, bit for bit what this entry has always returned.  A box
        that only a rare scale reaches is then carried by a handful of points: `prob` is off by orders of magnitude and `stderr`
        does not show it (an orthant at marginal level 1e-6 with dof = 3: seeds between 1e-15 and 2e-6 against 1.6e-7).
        "conditioned" (dof only, no shift;
        mlmc_copula_box_prob_tl_batch): component 0 of the caller's order LEADS: its score is drawn inside its limits by inversion
        of the t CDF with the exact weight W0 = T(upper_0 / F_00) - T(lower_0 / F_00), the mixing scale follows its law GIVEN that
        score (dof + 1 degrees of freedom), and the chain runs over components 1 .. M - 1: the relative error of the Gaussian chain
        at any depth.  Put the most constraining component first (`joint_probabilities` does).  streams are then M - 1 as before
        with streams[0] the lead's coordinate; the mixing scales are [R, B, n]
    :param return_lead: also return the lead scores v [R, B, n] (mixing="conditioned" only), after the mixing scales
    :return: JointProbability(prob [B], stderr [B], replicates [R, B], n, seeds)"""
    what = "copula_box_probabilities"
    dof = _check_dof(what, dof)
    lead = _check_mixing(what, mixing, dof, shift)
    if return_lead and not lead:
        raise ValueError(what + ': return_lead needs mixing="conditioned"')
    if dof is None and (mix_stream is not None or return_mixing):
        raise ValueError(what + ": mix_stream and return_mixing need dof (the Gaussian copula has no mixing variable)")
    f, lo, hi, shift = _box_problem(what, factor, lower, upper, shift, per_box=True)
    M, B = f.shape[-1], lo.shape[0]
    # one factor per box: the _pf_ entries, which take the distance of the factors (in doubles) behind them
    stride = (M * M,) if f.ndim == 3 else ()
    entry = lambda name: getattr(_lib.lib(), name + ("_pf_batch" if stride else "_batch"))          # noqa: E731
    n, seeds, first = _box_call_args(what, n, seeds, first)
    streams = _box_streams(what, streams, 2 if lead and M == 1 else M, qmc)          # the lead of M = 1 has a coordinate
    R = seeds.size
    flags = _lib.SAMPLE_SOBOL if qmc else 0
    mean = np.empty((R, B))
    if dof is None:
        (integrand,), kind = _output_arrays(device and return_integrand, [(R, B, n) if return_integrand else None])
        _lib.check(entry("mlmc_copula_box_prob")(M, _lib.ptr(f), *stride, B, _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(shift), R,
                                                 _lib.ptr(seeds), _lib.ptr(streams), first, n, flags, _lib.ptr(mean),
                                                 _lib.ptr(integrand), kind))
        result = _joint_probability(mean, n, seeds)
        return (result, integrand) if return_integrand else result
    if lead:
        # M = 1 has no chain coordinate but its lead has one; the entry takes [M] streams and does not read the last one for M > 1
        streams, mix_stream = _box_t_streams(what, dof, shift, streams, mix_stream, max(M - 1, 1), qmc)
        streams = np.ascontiguousarray(np.concatenate([streams, streams[-1:]])[:M], dtype=np.uint32)
        (integrand, s, v), kind = _output_arrays(device and (return_integrand or return_mixing or return_lead),
                                                 [(R, B, n) if return_integrand else None, (R, B, n) if return_mixing else None,
                                                  (R, B, n) if return_lead else None])
        _lib.check(entry("mlmc_copula_box_prob_tl")(M, _lib.ptr(f), *stride, B, _lib.ptr(lo), _lib.ptr(hi), dof, R, _lib.ptr(seeds),
                                                    _lib.ptr(streams), mix_stream, first, n, flags, _lib.ptr(mean),
                                                    _lib.ptr(integrand), _lib.ptr(s), _lib.ptr(v), kind))
        extra = tuple(a for a, want in ((integrand, return_integrand), (s, return_mixing), (v, return_lead)) if want)
        result = _joint_probability(mean, n, seeds)
        return (result,) + extra if extra else result
    streams, mix_stream = _box_t_streams(what, dof, shift, streams, mix_stream, M - 1, qmc)
    (integrand, s), kind = _output_arrays(device and (return_integrand or return_mixing),
                                          [(R, B, n) if return_integrand else None, (R, n) if return_mixing else None])
    _lib.check(entry("mlmc_copula_box_prob_t")(M, _lib.ptr(f), *stride, B, _lib.ptr(lo), _lib.ptr(hi), dof, R, _lib.ptr(seeds),
                                               _lib.ptr(streams), mix_stream, first, n, flags, _lib.ptr(mean),
                                               _lib.ptr(integrand), _lib.ptr(s), kind))
    extra = tuple(v for v, want in ((integrand, return_integrand), (s, return_mixing)) if want)
    result = _joint_probability(mean, n, seeds)
    return (result,) + extra if extra else result


def _joint_probability(replicates, n, seeds):
    """JointProbability of the seeds' means [R, B]"""
    R = replicates.shape[0]
    prob = replicates.mean(axis=0)
    stderr = np.std(replicates, axis=0, ddof=1) / np.sqrt(R) if R > 1 else np.full(replicates.shape[1], np.nan)
    return JointProbability(prob, stderr, replicates, n, seeds)


def _limit_scores(what, distrs, lo, hi):
    """Normal scores of the limits lo, hi [B, q] of q distributions: (z_lo, z_hi, keep, finish).  A limit that is infinite, or lies
    at or beyond an end of its distribution's domain, is an infinite score exactly and is set here, on the host; keep holds the
    components that some box constrains; finish() fills in the other limits in place through ONE `normal_scores` call"""
    B, q = lo.shape
    a, b = _domain_arrays(distrs)
    z_lo, z_hi = np.full((B, q), -np.inf), np.full((B, q), np.inf)
    z_lo[lo >= b[None, :]] = np.inf
    z_hi[hi <= a[None, :]] = -np.inf
    in_lo, in_hi = (lo > a[None, :]) & (lo < b[None, :]), (hi > a[None, :]) & (hi < b[None, :])
    keep = np.flatnonzero(np.any((z_lo > 0) | in_lo | (z_hi < 0) | in_hi, axis=0))           # constrained in some box

    def finish():
        if not (np.any(in_lo) or np.any(in_hi)):
            return
        mid = 0.5 * (a + b)
        x = np.concatenate([np.where(in_lo, lo, mid[None, :]), np.where(in_hi, hi, mid[None, :])], axis=0).T     # [q, 2 B]
        z = normal_scores([distrs[m] for m in keep], np.ascontiguousarray(x[keep]))
        z_lo[:, keep] = np.where(in_lo[:, keep], z[:, :B].T, z_lo[:, keep])
        z_hi[:, keep] = np.where(in_hi[:, keep], z[:, B:].T, z_hi[:, keep])
        if np.any(np.isnan(z_lo)) or np.any(np.isnan(z_hi)):
            raise ValueError(what + ": a limit has no normal score (a distribution without a positive finite mass?)")
    return z_lo, z_hi, keep, finish


def _box_dof(what, dof, mix_stream, given):
    """dof of a box entry in the components' own units, checked (None: the Gaussian copula)"""
    dof = _check_dof(what, dof)
    if dof is not None and given is not None:
        raise ValueError(what + ": dof together with given: this entry conditions under the Gaussian copula only (given k components "
                         "the others follow a t law with dof + k degrees of freedom); call conditional_probabilities / "
                         "conditional_event_samples")
    if dof is None and mix_stream is not None:
        raise ValueError(what + ": mix_stream needs dof (the Gaussian copula has no mixing variable)")
    return dof


def _conditional_dof(what, dof, mix_stream, given, M, plain):
    """dof of an entry of the conditional family in the components' own units, checked (None: the Gaussian copula): `given` is
    required (`plain` names the entry without it) and dof + the number of given components must stay within 192; touches no device"""
    if given is None:
        raise ValueError("{}: given is required (without given values: {})".format(what, plain))
    dof = _check_dof(what, dof)
    if dof is not None:
        _check_conditional_dof(what, dof, _parse_given(what, given, M)[0].size)
    if dof is None and mix_stream is not None:
        raise ValueError(what + ": mix_stream needs dof (the Gaussian copula has no mixing variable)")
    return dof


def lead_components(t_lo, t_hi, dof, candidates=None):
    """The lead component of each box for mixing="conditioned", on the host: the one with the smallest marginal probability
    T_dof(hi) - T_dof(lo), taken through the lower tail on either side as `t_scores` does (an upper-tail limit pair keeps its relative
    accuracy); ties go to the lowest index.
    :param t_lo, t_hi: [B, q] t scores of the limits
    :param candidates: None (all q) or the column indices to choose among
    :return: (lead [B] column indices, marginal [B, q] probabilities)"""
    from scipy.special import stdtr
    t_lo, t_hi = np.asarray(t_lo, dtype=np.float64), np.asarray(t_hi, dtype=np.float64)
    upper = t_lo > 0
    with np.errstate(invalid="ignore"):
        marg = np.where(upper, stdtr(dof, -t_lo) - stdtr(dof, -t_hi), stdtr(dof, t_hi) - stdtr(dof, t_lo))
    marg = np.where(t_lo < t_hi, marg, 0.0)
    cand = np.arange(marg.shape[1]) if candidates is None else np.asarray(candidates, dtype=np.int64)
    return cand[np.argmin(marg[:, cand], axis=1)], marg


def _lead_groups(lead):
    """[(lead column, box indices)] of the boxes grouped by their lead, ascending in the lead"""
    return [(int(c), np.flatnonzero(lead == c)) for c in np.unique(lead)]


BoxOrder = collections.namedtuple("BoxOrder", "perm factor lower upper shift ok")


def _box_order_problem(what, cov, lower, upper, shift, first):
    """(cov [M, M] or [B, M, M] symmetrised, lo, hi, shift or None, first int32 [B] or None) of `box_order`, checked"""
    c = np.array(cov, dtype=np.float64)
    if c.ndim not in (2, 3) or c.shape[-1] != c.shape[-2] or c.shape[-1] < 1 or c.shape[0] < 1:
        raise ValueError(what + ": the covariance must be [M, M] or one per box [B, M, M], got shape {}".format(c.shape))
    M = c.shape[-1]
    if M > _lib.BOX_PROB_MAX_M:
        raise ValueError(what + ": {} components exceed the cap of {}".format(M, _lib.BOX_PROB_MAX_M))
    if not np.all(np.isfinite(c)):
        raise ValueError(what + ": the covariance must be finite")
    c = np.ascontiguousarray(0.5 * (c + np.swapaxes(c, -1, -2)))
    lo, hi = _box_limits(what, lower, upper, M)
    if c.ndim == 3:
        if lo.shape[0] == 1 and c.shape[0] > 1:
            lo, hi = np.repeat(lo, c.shape[0], axis=0), np.repeat(hi, c.shape[0], axis=0)
        if lo.shape[0] != c.shape[0]:
            raise ValueError(what + ": {} covariances, one per box, but the limits hold {} boxes".format(c.shape[0], lo.shape[0]))
    lo, hi, shift = _box_shift(what, lo, hi, shift)
    B = lo.shape[0]
    if first is not None:
        fi = np.asarray(first)
        if fi.dtype.kind not in "iu" or fi.ndim > 1:
            raise ValueError(what + ": first must hold integers: a component per box, -1 for a free lead")
        try:
            fi = np.broadcast_to(fi, (B,))
        except ValueError:
            raise ValueError(what + ": first {} does not broadcast to the {} boxes".format(fi.shape, B)) from None
        bad = np.flatnonzero((fi < -1) | (fi >= M))
        if bad.size:
            raise ValueError(what + ": first of box {} is {}: neither -1 nor a component below {}".format(int(bad[0]), int(fi[bad[0]]), M))
        first = np.ascontiguousarray(fi, dtype=np.int32)
    return c, lo, hi, shift, first


def box_order(cov, lower, upper, shift=None, first=None, check=True):
    """Genz's VARIABLE REORDERING for `copula_box_probabilities`, for B boxes through ONE device call
    (mlmc_copula_box_order_batch; Genz 1992, Gibson, Glasbey and Elston 1994): a greedy pivoted Cholesky factorisation of the
    covariance of the scores.  At every step the remaining component with the smallest expected conditional width
    Phi(b) - Phi(a) (given the expected values of the components already placed) is integrated next; ties go to the lowest
    original index.  The probability of a box does not depend on the order of its components; the variance of the chain's estimate
    does, by orders of magnitude where the limits are heterogeneous and the components correlated.  Everything is in NORMAL-SCORE
    space.  The result goes to `copula_box_probabilities(order.factor, order.lower, order.upper, ..., shift=order.shift)`:
    one factor per box.
    :param cov: [M, M] symmetric positive definite (it is symmetrised), or one per box [B, M, M].  M <= 128
    :param lower, upper: broadcast to [B, M], +-inf allowed
    :param shift: None or the mean of the scores, broadcast to [B, M]
    :param first: None, or integers broadcast to [B]: the component that is forced to lead its box, -1 for a free choice
    :param check: raise ValueError for a box whose factorisation met a pivot that is not positive (names the box); False: see `ok`
    :return: BoxOrder(perm [B, M] int32: perm[b, i] is the original component at position i; factor [B, M, M]: the lower-triangular
        factor of cov[perm][:, perm]; lower, upper [B, M] and shift ([B, M] or None) permuted; ok [B] bool)"""
    what = "box_order"
    problem = _box_order_problem(what, cov, lower, upper, shift, first)
    # host arrays, all of them: this entry takes no device memory
    c = np.ascontiguousarray(problem[0])
    lo = np.ascontiguousarray(problem[1])
    hi = np.ascontiguousarray(problem[2])
    sh = None if problem[3] is None else np.ascontiguousarray(problem[3])
    lead = None if problem[4] is None else np.ascontiguousarray(problem[4])
    B, M = lo.shape
    perm = np.empty((B, M), dtype=np.int32)
    factor = np.empty((B, M, M))
    ok = np.empty(B, dtype=np.int32)
    _lib.check(_lib.lib().mlmc_copula_box_order_batch(M, _lib.ptr(c), M * M if c.ndim == 3 else 0, B, _lib.ptr(lo), _lib.ptr(hi),
                                                     _lib.ptr(sh), _lib.ptr(lead), _lib.ptr(perm), _lib.ptr(factor), _lib.ptr(ok)))
    fine = ok != 0
    if check and not np.all(fine):
        raise ValueError(what + ": box {}: the covariance is not positive definite (a pivot of the factorisation is not positive)".format(
            int(np.flatnonzero(~fine)[0])))
    take = lambda x: None if x is None else np.ascontiguousarray(np.take_along_axis(x, perm.astype(np.int64), axis=1))   # noqa: E731
    return BoxOrder(perm, factor, take(lo), take(hi), take(sh), fine)


def _check_order(what, order, out_of_scope=None):
    """True for order="genz", checked; out_of_scope: why this entry cannot reorder (it then raises for "genz")"""
    if order not in ("natural", "genz"):
        raise ValueError(what + ': order must be "natural" or "genz", got {!r}'.format(order))
    if order == "genz" and out_of_scope:
        raise ValueError(what + ': order="genz" is out of scope here: ' + out_of_scope)
    return order == "genz"


def joint_probabilities(distrs, lower, upper, n, seeds, corr=None, factor=None, given=None, streams=None, first=0, qmc=True,
                        return_integrand=False, device=False, dof=None, mix_stream=None, mixing="plain", order="natural",
                        return_order=False):
    """Joint box probabilities P(lower_m < X_m < upper_m for all m) under the Gaussian copula of `joint_samples`, for B boxes in
    the components' own units through `copula_box_probabilities`; with `given`, conditional on the given values of some
    components as in `conditional_samples`.  A limit that is +-inf or lies at or beyond an end of its distribution's domain is an
    infinite score exactly; every other limit goes through ONE `normal_scores` call.  Components that no box of the call
    constrains are dropped before the factorisation (the marginal law of a Gaussian sub-vector is the sub-matrix of its
    correlation), so two constrained components out of 64 are a two-dimensional problem.
    :param lower, upper: broadcast to [B, M]; with `given` to [B, q] over the q components that are not given, ascending
    :param corr: correlation matrix [M, M] of the normal scores (goes through `correlation_factor`, as in `joint_samples`)
    :param factor: or a factor [M, K] with rows of unit norm: F F^T is taken as the correlation.  Exactly one of the two
    :param given: None, or the mapping of `conditional_samples`; arrays [B] pair with the boxes (one box pairs with all sets)
    :param streams: per coordinate of the REDUCED problem (constrained components - 1)
    :param n, seeds, first, qmc, return_integrand, device: as in `copula_box_probabilities`
    :param dof, mix_stream: the STUDENT-T copula of `joint_samples(dof=...)` in the place of the Gaussian one: the normal scores of
        the limits go to t scores on the host (`t_scores`) and the box goes through `copula_box_probabilities(dof=...)`; corr /
        factor are then the t copula's correlation matrix (`Estimate.estimate_quadrant_correlation` estimates it).  Dropping the
        unconstrained components stays valid: a sub-vector of a multivariate t is a t with the same dof and the sub-matrix.  None or
        np.inf: the Gaussian copula, bit for bit.  Not together with `given`: that is `conditional_probabilities`
    :param mixing: "plain" (default): bit for bit what this entry has always returned; a box that only a rare mixing scale reaches
        (marginal levels of 1e-6 at dof = 3) then comes out orders of magnitude too small with a `stderr` that does not show it.
        "conditioned" (dof only): the conditioned lead of `copula_box_probabilities`.  After the unconstrained components are
        dropped, the lead of each box is the component with the smallest marginal probability (`lead_components`; ties: the lowest
        index); boxes are grouped by lead with one device call per group, the correlation permuted lead-first and refactored on the
        host.  streams[0] is then the lead's coordinate, streams[i] that of the i-th other constrained component, ascending.  Out of
        scope: `given` (raises: the conditional family keeps plain mixing); the order BEHIND the lead is the caller's unless
        order="genz"
    :param order: "natural" (default): the constrained components are integrated in the caller's order (behind the lead, under
        mixing="conditioned"), bit for bit what this entry has always returned.  "genz": Genz's variable reordering (`box_order`)
        of the constrained components of EVERY box, then ONE device call with one factor per box.  The probability needs no
        un-permuting.  With `given` the conditional covariance F_c F_c^T and the conditional means go to `box_order`.  Under `dof`
        the ORDER is computed on the NORMAL scores of the limits with the same correlation matrix (the t scores of deep limits are
        far too large for normal widths to tell the components apart); the chain then runs on the t scores in that order.  Every
        order is unbiased: this one is a heuristic for the variance.  With mixing="conditioned" the lead of `lead_components` is
        forced to position 0 and the others are ordered behind it, so the groups by lead collapse into one call.  streams[i]
        belongs to POSITION i of the order: the lowest Sobol' dimensions go to the components integrated first.  It helps where the
        limits are heterogeneous and the components correlated; independent components gain nothing (their widths do not depend on
        the points)
    :param return_order: also return, last, perm [B, k] int64: the ORIGINAL index (into `distrs`) of the component at each position
        of the chain of every box, k the number of constrained components
    :return: JointProbability; a call that constrains nothing returns ones without a device call (and no integrand: None)"""
    return _joint_probabilities("joint_probabilities", False, distrs, lower, upper, n, seeds, corr, factor, given, streams, first, qmc,
                                return_integrand, device, dof, mix_stream, mixing, order, return_order)


def _joint_probabilities(what, conditional, distrs, lower, upper, n, seeds, corr, factor, given, streams, first, qmc, return_integrand,
                         device, dof, mix_stream, mixing="plain", order="natural", return_order=False):
    """the one body of `joint_probabilities` and `conditional_probabilities` (conditional: the second one, where dof with given
    components goes through `conditional_box_probabilities`); the argument errors come in the order they have always had"""
    distrs = list(distrs)
    M = len(distrs)
    if M == 0:
        raise ValueError(what + ": no distributions")
    if conditional:
        dof = _conditional_dof(what, dof, mix_stream, given, M, "joint_probabilities")
    else:
        dof = _box_dof(what, dof, mix_stream, given)
    lead = _check_mixing(what, mixing, dof, None, given)
    genz = _check_order(what, order, "a conditional law of the t copula (the _tc_ entries) keeps one shared factor"
                        if conditional and dof is not None else None)
    if (corr is None) == (factor is None):
        raise ValueError(what + ": exactly one of corr and factor must be given")
    n, seeds, first = _box_call_args(what, n, seeds, first)
    _common_quadrature(what, distrs)
    if factor is not None:
        fac = np.asarray(factor, dtype=np.float64)
        if fac.ndim != 2 or fac.shape[0] != M or fac.shape[1] < 1 or not np.all(np.isfinite(fac)):
            raise ValueError(what + ": the factor must be a finite [M, K] matrix with M = {} distributions".format(M))
        corr = fac @ fac.T
    corr = np.array(corr, dtype=np.float64)
    if corr.shape != (M, M):
        raise ValueError(what + ": corr must be [M, M] with M = {} distributions, got shape {}".format(M, corr.shape))
    if given is not None:
        observed, values, _ = _parse_given(what, given, M)
        free = np.setdiff1d(np.arange(M, dtype=np.int64), observed)
    else:
        observed, values, free = np.zeros(0, dtype=np.int64), np.zeros((0, 1)), np.arange(M, dtype=np.int64)
    q = free.size
    lo, hi = _box_limits(what, lower, upper, q, "q" if given is not None else "M")
    B = lo.shape[0]
    Bg = values.shape[1]
    if Bg != 1 and B != 1 and Bg != B:
        raise ValueError(what + ": the arrays of given hold {} sets, there are {} boxes".format(Bg, B))
    if B == 1 and Bg > 1:
        lo, hi = np.repeat(lo, Bg, axis=0), np.repeat(hi, Bg, axis=0)
        B = Bg
    z_lo, z_hi, keep, finish = _limit_scores(what, [distrs[m] for m in free], lo, hi)
    streams = _box_streams(what, streams, 2 if lead and keep.size <= 1 else max(keep.size, 1), qmc)
    if dof is not None:
        streams, mix_stream = _box_t_streams(what, dof, None, streams, mix_stream, max(keep.size - 1, 1 if lead else 0), qmc)
    if keep.size > _lib.BOX_PROB_MAX_M:
        raise ValueError(what + ": {} constrained components exceed the cap of {}".format(keep.size, _lib.BOX_PROB_MAX_M))

    def with_order(out, perm):
        if not return_order:
            return out
        return out + (perm,) if type(out) is tuple else (out, perm)

    if keep.size == 0:
        ones = _joint_probability(np.ones((seeds.size, B)), n, seeds)
        return with_order((ones, None) if return_integrand else ones, np.zeros((B, 0), dtype=np.int64))
    finish()
    comp = free[keep]
    if genz:
        # the order of every box from the NORMAL scores of its limits (under dof too: a heuristic, every order is unbiased), then
        # one device call with one factor per box
        n_lo, n_hi = z_lo[:, keep], z_hi[:, keep]
        if observed.size:
            _, _, _, _, (_, fc, _), mu, _ = _conditioning(what, distrs, given, corr, None)
            cov = (fc @ fc.T)[np.ix_(keep, keep)]
            shift = np.ascontiguousarray(np.broadcast_to(mu[:, keep], (B, keep.size)))
        else:
            low = correlation_factor(corr[np.ix_(comp, comp)])[0]
            cov, shift = low @ low.T, None
        force = None
        if dof is not None:
            t_lo, t_hi = t_scores(n_lo, dof), t_scores(n_hi, dof)
            if lead:
                force = lead_components(t_lo, t_hi, dof)[0]
        ordered = box_order(cov, n_lo, n_hi, shift=shift, first=force)
        at = ordered.perm.astype(np.int64)
        if dof is None:
            b_lo, b_hi = ordered.lower, ordered.upper
        else:
            b_lo, b_hi = np.take_along_axis(t_lo, at, axis=1), np.take_along_axis(t_hi, at, axis=1)
        out = copula_box_probabilities(ordered.factor, b_lo, b_hi, n, [int(s) for s in seeds], shift=ordered.shift, streams=streams,
                                       first=first, qmc=qmc, return_integrand=return_integrand, device=device, dof=dof,
                                       mix_stream=mix_stream, mixing=mixing)
        return with_order(out, comp[at])
    if dof is not None:
        z_lo, z_hi = t_scores(z_lo, dof), t_scores(z_hi, dof)
    if lead:
        # one device call per lead: the correlation of the constrained components permuted lead-first and refactored
        t_lo, t_hi = z_lo[:, keep], z_hi[:, keep]
        R = seeds.size
        replicates = np.empty((R, B))
        integrand = None
        perm = np.empty((B, keep.size), dtype=np.int64)
        for c, boxes in _lead_groups(lead_components(t_lo, t_hi, dof)[0]):
            order = np.concatenate([[c], np.delete(np.arange(keep.size), c)])
            comp = free[keep][order]
            perm[boxes] = comp
            low = correlation_factor(corr[np.ix_(comp, comp)])[0]
            out = copula_box_probabilities(low, t_lo[np.ix_(boxes, order)], t_hi[np.ix_(boxes, order)], n, [int(s) for s in seeds],
                                           streams=streams, first=first, qmc=qmc, return_integrand=return_integrand, device=device,
                                           dof=dof, mix_stream=mix_stream, mixing=mixing)
            res, f = out if return_integrand else (out, None)
            replicates[:, boxes] = res.replicates
            if return_integrand:
                if integrand is None:
                    integrand = f if boxes.size == B else (f.new_empty((R, B, n)) if device else np.empty((R, B, n)))
                if boxes.size != B:
                    integrand[:, boxes.tolist() if device else boxes, :] = f
        result = _joint_probability(replicates, n, seeds)
        return with_order((result, integrand) if return_integrand else result, perm)
    natural = np.ascontiguousarray(np.broadcast_to(comp, (B, keep.size)))
    if observed.size and dof is not None:
        cond = conditional_factor(corr, observed, return_observed=True)
        _, _, _, _, (_, fc, _), mu, r = _conditioning(what, distrs, given, None, cond, dof)
        cov = fc @ fc.T
        low = np.linalg.cholesky(cov[np.ix_(keep, keep)])
        shift = np.ascontiguousarray(np.broadcast_to(mu[:, keep], (B, keep.size)))
        return with_order(conditional_box_probabilities(low, z_lo[:, keep], z_hi[:, keep], n, [int(s) for s in seeds], dof,
                                                        dof_mix=dof + observed.size, shift=shift, scale=np.broadcast_to(r, (B,)),
                                                        streams=streams, first=first, qmc=qmc, return_integrand=return_integrand,
                                                        device=device, mix_stream=mix_stream), natural)
    if observed.size:
        _, _, _, _, (_, fc, _), mu, _ = _conditioning(what, distrs, given, corr, None)
        cov = fc @ fc.T
        low = np.linalg.cholesky(cov[np.ix_(keep, keep)])
        shift = np.ascontiguousarray(np.broadcast_to(mu[:, keep], (B, keep.size)))
    else:
        low = correlation_factor(corr[np.ix_(free[keep], free[keep])])[0]
        shift = None
    return with_order(copula_box_probabilities(low, z_lo[:, keep], z_hi[:, keep], n, [int(s) for s in seeds], shift=shift,
                                               streams=streams, first=first, qmc=qmc, return_integrand=return_integrand, device=device,
                                               dof=dof, mix_stream=mix_stream), natural)


def joint_probabilities_over_correlations(distrs, lower, upper, n, seeds, corrs, first=0, qmc=True, dof=None, order="natural"):
    """`joint_probabilities(distrs, lower, upper, n, seeds, corr=corrs[c], dof=dof)` for EVERY correlation matrix of corrs [C, M, M]
    through ONE device call: the limits map to scores once (they do not depend on the correlation), every matrix is factored on the
    host, and the C x B (correlation, box) pairs are the boxes of one `copula_box_probabilities` call with one factor per box.  A
    replicate depends on (factor, box, seed, streams, first, n, qmc) alone, so result c is bit for bit that of the single call.
    Made for bootstrap replicates of a correlation matrix (Estimate.bootstrap_joint_probability).
    :param corrs: [C, M, M]; corrs[0] must factor (its error is raised); another matrix whose `correlation_factor` raises is not ok
    :param order: "natural" or "genz" (`box_order` for every pair, still one chain call), as in `joint_probabilities`
    :return: (results: a list of C JointProbability, None where not ok; ok [C] bool)"""
    what = "joint_probabilities_over_correlations"
    distrs = list(distrs)
    M = len(distrs)
    if M == 0:
        raise ValueError(what + ": no distributions")
    dof = _box_dof(what, dof, None, None)
    genz = _check_order(what, order)
    n, seeds, first = _box_call_args(what, n, seeds, first)
    _common_quadrature(what, distrs)
    corrs = np.asarray(corrs, dtype=np.float64)
    if corrs.ndim != 3 or corrs.shape[0] < 1 or corrs.shape[1:] != (M, M):
        raise ValueError(what + ": corrs must be [C, M, M] with M = {} distributions, got shape {}".format(M, corrs.shape))
    lo, hi = _box_limits(what, lower, upper, M)
    B, C = lo.shape[0], corrs.shape[0]
    z_lo, z_hi, keep, finish = _limit_scores(what, distrs, lo, hi)
    streams = _box_streams(what, None, max(keep.size, 1), qmc)
    mix_stream = None
    if dof is not None:
        streams, mix_stream = _box_t_streams(what, dof, None, streams, None, max(keep.size - 1, 0), qmc)
    if keep.size > _lib.BOX_PROB_MAX_M:
        raise ValueError(what + ": {} constrained components exceed the cap of {}".format(keep.size, _lib.BOX_PROB_MAX_M))
    ok = np.ones(C, dtype=bool)
    if keep.size == 0:
        return [_joint_probability(np.ones((seeds.size, B)), n, seeds) for _ in range(C)], ok
    finish()
    n_lo, n_hi = z_lo[:, keep], z_hi[:, keep]
    lows = []
    for c in range(C):
        try:
            lows.append(correlation_factor(corrs[c][np.ix_(keep, keep)])[0])
        except Exception:
            if c == 0:
                raise
            ok[c] = False
    lows = np.repeat(np.array(lows), B, axis=0)                                     # pair (c, b) at c * B + b
    b_lo, b_hi = np.tile(n_lo, (int(ok.sum()), 1)), np.tile(n_hi, (int(ok.sum()), 1))
    if genz:
        ordered = box_order(lows @ np.swapaxes(lows, 1, 2), b_lo, b_hi)
        lows, at = ordered.factor, ordered.perm.astype(np.int64)
        b_lo, b_hi = np.take_along_axis(b_lo, at, axis=1), np.take_along_axis(b_hi, at, axis=1)
    if dof is not None:
        b_lo, b_hi = t_scores(b_lo, dof), t_scores(b_hi, dof)
    reps = copula_box_probabilities(lows, b_lo, b_hi, n, [int(s) for s in seeds], streams=streams, first=first, qmc=qmc, dof=dof,
                                    mix_stream=mix_stream).replicates
    # the statistics of a result from an array laid out as the single call has it
    results, k = [None] * C, 0
    for c in np.flatnonzero(ok):
        results[c] = _joint_probability(np.ascontiguousarray(reps[:, k * B:(k + 1) * B]), n, seeds)
        k += 1
    return results, ok


BoxDraws = collections.namedtuple("BoxDraws", "z u weights prob")


def copula_box_draws(factor, lower, upper, n, seeds, shift=None, streams=None, first=0, qmc=True, device=False, dof=None,
                     mix_stream=None, return_mixing=False, mixing="plain", return_lead=False):
    """Scenarios of Y = shift + F z GIVEN lower < Y < upper, for B boxes and R seeds through ONE device call
    (mlmc_copula_box_draws_batch): the conditioned normals of the chain of `copula_box_probabilities` are a sequential importance
    sample of the truncated normal vector (the GHK sampler).  Every point is a scenario inside the box; its weight is the
    integrand of the box probability, so sum(weights * g(z)) / sum(weights) estimates E[g(Y) | box] and the mean of the weights
    is the probability itself.  Everything is in SCORE space (`event_samples` works in the components' own units).  The weights
    vary least when the components that the box constrains come first in the chain; a box that constrains nothing gives weights
    exactly 1 and plain joint draws.  A value depends on (factor, box, seed, streams, point index, qmc) alone.
    :param factor, lower, upper, n, seeds, shift, first, qmc: as in `copula_box_probabilities`
    :param streams: one stream (qmc: Sobol' dimension below 1024) per coordinate, M of them (the last draws the last component);
        default: i.  The weights and `prob` are those of `copula_box_probabilities` with the first M - 1 of them, bit for bit
    :param device: return z, u and the weights as float64 torch device tensors
    :return: BoxDraws(z [R, B, M, n], u [R, B, M, n], weights [R, B, n], prob): the scores, lower <= z <= upper; u = Phi(z) clamped
        to [2^-53, 1 - 2^-53] as in `joint_samples`; prob the JointProbability of the event
    :param dof, mix_stream: the Student-t law of `copula_box_probabilities` (mlmc_copula_box_draws_t_batch): limits and the returned
        z are then T scores, z = clip((chain's normal) * s, lower, upper), and u = T_dof(z) of `student_t_cdf`, clamped alike.  By
        default the mixing stream is 0 and coordinate i takes stream i + 1, so weights and `prob` are again those of
        `copula_box_probabilities` with the same dof, bit for bit.  Not together with `shift` (`conditional_box_draws`)
    :param return_mixing: return (BoxDraws, s [R, n]) (dof only)
    :param mixing: "plain" (default, bit for bit as before) or "conditioned" (dof only, no shift; mlmc_copula_box_draws_tl_batch):
        the conditioned lead of `copula_box_probabilities`: component 0 leads, streams[0] is its coordinate, row 0 of z is
        clip(v F_00, lower_0, upper_0) and the mixing scales are [R, B, n].  Weights and `prob` are those of
        `copula_box_probabilities(mixing="conditioned")`, bit for bit
    :param return_lead: append the lead scores v [R, B, n] to the returned tuple (mixing="conditioned" only)"""
    what = "copula_box_draws"
    dof = _check_dof(what, dof)
    lead = _check_mixing(what, mixing, dof, shift)
    if return_lead and not lead:
        raise ValueError(what + ': return_lead needs mixing="conditioned"')
    if dof is None and (mix_stream is not None or return_mixing):
        raise ValueError(what + ": mix_stream and return_mixing need dof (the Gaussian copula has no mixing variable)")
    f, lo, hi, shift = _box_problem(what, factor, lower, upper, shift)
    M, B = f.shape[0], lo.shape[0]
    n, seeds, first = _box_call_args(what, n, seeds, first)
    streams = _box_streams(what, streams, M + 1, qmc)
    R = seeds.size
    flags = _lib.SAMPLE_SOBOL if qmc else 0
    mean = np.empty((R, B))
    if dof is None:
        (z, u, w), kind = _output_arrays(device, [(R, B, M, n), (R, B, M, n), (R, B, n)])
        _lib.check(_lib.lib().mlmc_copula_box_draws_batch(M, _lib.ptr(f), B, _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(shift), R,
                                                         _lib.ptr(seeds), _lib.ptr(streams), first, n, flags, _lib.ptr(mean), _lib.ptr(w),
                                                         _lib.ptr(z), _lib.ptr(u), kind))
        return BoxDraws(z, u, w, _joint_probability(mean, n, seeds))
    streams, mix_stream = _box_t_streams(what, dof, shift, streams, mix_stream, M, qmc)
    if lead:
        (z, u, w, s, v), kind = _output_arrays(device, [(R, B, M, n), (R, B, M, n), (R, B, n), (R, B, n) if return_mixing else None,
                                                        (R, B, n) if return_lead else None])
        _lib.check(_lib.lib().mlmc_copula_box_draws_tl_batch(M, _lib.ptr(f), B, _lib.ptr(lo), _lib.ptr(hi), dof, R, _lib.ptr(seeds),
                                                            _lib.ptr(streams), mix_stream, first, n, flags, _lib.ptr(mean), _lib.ptr(w),
                                                            _lib.ptr(z), _lib.ptr(u), _lib.ptr(s), _lib.ptr(v), kind))
        box = BoxDraws(z, u, w, _joint_probability(mean, n, seeds))
        extra = tuple(a for a, want in ((s, return_mixing), (v, return_lead)) if want)
        return (box,) + extra if extra else box
    (z, u, w, s), kind = _output_arrays(device, [(R, B, M, n), (R, B, M, n), (R, B, n), (R, n) if return_mixing else None])
    _lib.check(_lib.lib().mlmc_copula_box_draws_t_batch(M, _lib.ptr(f), B, _lib.ptr(lo), _lib.ptr(hi), dof, R, _lib.ptr(seeds),
                                                       _lib.ptr(streams), mix_stream, first, n, flags, _lib.ptr(mean), _lib.ptr(w),
                                                       _lib.ptr(z), _lib.ptr(u), _lib.ptr(s), kind))
    box = BoxDraws(z, u, w, _joint_probability(mean, n, seeds))
    return (box, s) if return_mixing else box


def _conditional_box_problem(what, factor, lower, upper, dof, dof_mix, shift, scale):
    """(factor, lo, hi, shift [B, M] or None, scale [B] or None, dof, dof_mix) of a conditional box call under the t copula,
    checked; touches no device"""
    dof = _check_dof(what, dof)
    if dof is None:
        raise ValueError(what + ": dof must be finite, in [1, 64] (the Gaussian copula: copula_box_probabilities / copula_box_draws "
                         "with a shift)")
    dof_mix = dof if dof_mix is None else _check_dof_mix(what, dof_mix)
    f, lo, hi, shift = _box_problem(what, factor, lower, upper, shift)
    B = lo.shape[0]
    if scale is not None:
        sc = np.asarray(scale, dtype=np.float64)
        try:
            sc = np.ascontiguousarray(np.broadcast_to(sc, (B,)))
        except ValueError:
            raise ValueError(what + ": scale {} does not broadcast to [B] = {}".format(sc.shape, (B,))) from None
        if not np.all(np.isfinite(sc) & (sc > 0)):
            raise ValueError(what + ": the scale must be finite and positive")
        scale = sc
    return f, lo, hi, shift, scale, dof, dof_mix


def conditional_box_probabilities(factor, lower, upper, n, seeds, dof, dof_mix=None, shift=None, scale=None, streams=None, first=0,
                                  qmc=True, return_integrand=False, device=False, mix_stream=None, return_mixing=False):
    """P(lower < Y < upper) for a CONDITIONAL law of the Student-t copula, Y = shift + scale s_c F z: z standard normal,
    s_c = conditional_mixing_scale(p0, dof_mix) one mixing scale per point, for B boxes and R seeds through ONE device call
    (mlmc_copula_box_prob_tc_batch).  Given the t scores y_O of p components, the t scores of the others are multivariate t with
    dof_mix = dof + p degrees of freedom, location shift = W y_O and scale matrix scale^2 F F^T, scale^2 = (dof + d) / (dof + p),
    d = |L_OO^-1 y_O|^2 (`conditional_factor(..., return_observed=True)`), so
        P(lower < Y < upper) = E_sc[P((lower - shift) / (scale s_c) < F z < (upper - shift) / (scale s_c))],
    the chain of `copula_box_probabilities(dof=...)` on these quotients.  Everything is in T-SCORE space (`conditional_probabilities`
    works in the components' own units).  With shift None, scale None and dof_mix == dof the result is bit for bit that of
    `copula_box_probabilities(dof=...)`.
    :param factor, lower, upper, n, seeds, first, qmc, return_integrand, device: as in `copula_box_probabilities`
    :param dof: the degrees of freedom of the copula, a float in [1, 64]
    :param dof_mix: those of the mixing variable, a float in [1, 192]; default: dof
    :param shift: None or the location, broadcast to [B, M], finite
    :param scale: None (ones) or the scale of each box, broadcast to [B], finite and positive
    :param streams, mix_stream: as in `copula_box_probabilities(dof=...)`: by default the mixing variable takes stream 0 and chain
        coordinate i stream i + 1; with explicit `streams`, mix_stream must be given and differ from all of them
    :param return_mixing: also return the mixing scales s_c [R, n], after the integrand
    :return: JointProbability(prob [B], stderr [B], replicates [R, B], n, seeds)"""
    what = "conditional_box_probabilities"
    f, lo, hi, shift, scale, dof, dof_mix = _conditional_box_problem(what, factor, lower, upper, dof, dof_mix, shift, scale)
    M, B = f.shape[0], lo.shape[0]
    n, seeds, first = _box_call_args(what, n, seeds, first)
    streams = _box_streams(what, streams, M, qmc)
    R = seeds.size
    flags = _lib.SAMPLE_SOBOL if qmc else 0
    mean = np.empty((R, B))
    streams, mix_stream = _box_t_streams(what, dof, None, streams, mix_stream, M - 1, qmc)
    (integrand, s), kind = _output_arrays(device and (return_integrand or return_mixing),
                                          [(R, B, n) if return_integrand else None, (R, n) if return_mixing else None])
    _lib.check(_lib.lib().mlmc_copula_box_prob_tc_batch(M, _lib.ptr(f), B, _lib.ptr(lo), _lib.ptr(hi), dof, dof_mix, _lib.ptr(shift),
                                                       _lib.ptr(scale), R, _lib.ptr(seeds), _lib.ptr(streams), mix_stream, first, n,
                                                       flags, _lib.ptr(mean), _lib.ptr(integrand), _lib.ptr(s), kind))
    extra = tuple(v for v, want in ((integrand, return_integrand), (s, return_mixing)) if want)
    result = _joint_probability(mean, n, seeds)
    return (result,) + extra if extra else result


def conditional_box_draws(factor, lower, upper, n, seeds, dof, dof_mix=None, shift=None, scale=None, streams=None, first=0, qmc=True,
                          device=False, mix_stream=None, return_mixing=False):
    """Scenarios of the conditional t law of `conditional_box_probabilities` GIVEN lower < Y < upper, through ONE device call
    (mlmc_copula_box_draws_tc_batch): the GHK sampler of `copula_box_draws(dof=...)` on the limits (lower - shift) / (scale s_c);
    the returned t score is z = clip(shift + (chain's normal) * (scale s_c), lower, upper) and u = T_dof(z) of `student_t_cdf`
    with the COPULA's dof (the marginal law of a component is t with dof, not dof_mix), clamped to [2^-53, 1 - 2^-53].  Weights and
    `prob` are those of `conditional_box_probabilities` bit for bit under default streams.
    :param streams: one per coordinate, M of them; the other arguments as in `conditional_box_probabilities`
    :param return_mixing: return (BoxDraws, s_c [R, n])
    :return: BoxDraws(z [R, B, M, n], u [R, B, M, n], weights [R, B, n], prob)"""
    what = "conditional_box_draws"
    f, lo, hi, shift, scale, dof, dof_mix = _conditional_box_problem(what, factor, lower, upper, dof, dof_mix, shift, scale)
    M, B = f.shape[0], lo.shape[0]
    n, seeds, first = _box_call_args(what, n, seeds, first)
    streams = _box_streams(what, streams, M + 1, qmc)
    R = seeds.size
    flags = _lib.SAMPLE_SOBOL if qmc else 0
    mean = np.empty((R, B))
    streams, mix_stream = _box_t_streams(what, dof, None, streams, mix_stream, M, qmc)
    (z, u, w, s), kind = _output_arrays(device, [(R, B, M, n), (R, B, M, n), (R, B, n), (R, n) if return_mixing else None])
    _lib.check(_lib.lib().mlmc_copula_box_draws_tc_batch(M, _lib.ptr(f), B, _lib.ptr(lo), _lib.ptr(hi), dof, dof_mix, _lib.ptr(shift),
                                                        _lib.ptr(scale), R, _lib.ptr(seeds), _lib.ptr(streams), mix_stream, first, n,
                                                        flags, _lib.ptr(mean), _lib.ptr(w), _lib.ptr(z), _lib.ptr(u), _lib.ptr(s), kind))
    box = BoxDraws(z, u, w, _joint_probability(mean, n, seeds))
    return (box, s) if return_mixing else box


def conditional_probabilities(distrs, lower, upper, given, n, seeds, corr=None, factor=None, dof=None, streams=None, first=0, qmc=True,
                              return_integrand=False, device=False, mix_stream=None, order="natural", return_order=False):
    """Joint box probabilities of the components that are NOT in `given`, conditional on the given values of the others: the
    probability member of the conditional family (`conditional_samples`, `conditional_quantiles`, `conditional_cdfs`).  With dof
    None (or np.inf) this is `joint_probabilities(given=...)`, bit for bit, through the same body.  With dof, a float in [1, 64],
    the copula is the STUDENT-T copula of `joint_samples(dof=...)`: the limits go to t scores, the given values to t scores y_O, and
    given them the others are multivariate t with dof + p degrees of freedom, location W y_O and scale matrix r^2 F_c F_c^T
    (`conditional_samples(dof=...)`), so an extreme given value WIDENS the law of the others; the box goes through
    `conditional_box_probabilities` with shift = mu, scale = r, dof_mix = dof + p.  Components that no box constrains are dropped
    (a sub-vector of a multivariate t keeps its degrees of freedom).  dof + p must not exceed 192.
    :param lower, upper: broadcast to [B, q] over the q components that are not given, ascending, in their own units
    :param given: the mapping of `conditional_samples` (required); arrays [B] pair with the boxes (one box pairs with all sets)
    :param corr, factor: as in `joint_probabilities`; with dof the t copula's correlation matrix
    :param streams, mix_stream: per coordinate of the REDUCED problem, and the mixing stream, as in `joint_probabilities(dof=...)`
    :param order, return_order: as in `joint_probabilities`.  order="genz" works under the Gaussian copula (dof None); with dof it
        raises: the conditional t entries keep one shared factor
    :return: JointProbability; a call that constrains nothing returns ones without a device call (and no integrand: None)"""
    return _joint_probabilities("conditional_probabilities", True, distrs, lower, upper, n, seeds, corr, factor, given, streams, first,
                                qmc, return_integrand, device, dof, mix_stream, "plain", order, return_order)


def conditional_event_samples(distrs, lower, upper, given, n, seeds, corr=None, factor=None, streams=None, first=0, qmc=True,
                              device=False, dof=None, mix_stream=None, order="natural"):
    """Joint scenarios of ALL components GIVEN the event lower_m < X_m < upper_m AND the given values of some components.  With dof
    None (or np.inf) this is `event_samples(given=...)`, bit for bit, through the same body.  With dof the copula is the Student-t
    copula, as in `conditional_probabilities`: the chain order of `event_samples`, `conditional_box_draws` with shift = mu,
    scale = r and dof_mix = dof + p, and one `quantiles` call on its u.  Rows of given components hold the given values (uniforms:
    Fhat of them).  Under default streams `prob` is bit for bit that of `conditional_probabilities` where no component is dropped
    there.
    :param lower, upper: broadcast to [B, M] in the components' own units; a given component must not be constrained
    :param given: the mapping of `conditional_samples` (required)
    :param order: "natural"; "genz" raises, as in `event_samples`
    :return: EventScenarios"""
    _check_order("conditional_event_samples", order, _DRAWS_ORDER)
    return _event_samples("conditional_event_samples", True, distrs, lower, upper, n, seeds, corr, factor, given, streams, first, qmc,
                          device, dof, mix_stream)


def _event_order(constrained, q):
    """chain order of q components: the constrained ones first, ascending, then the rest, ascending.  With a constrained component
    behind an unconstrained one the weights carry the whole conditioning of the earlier draws (a tenth of the effective sample
    size in the example of DESIGN 3.5.18); in front, one constrained component alone has constant weights"""
    constrained = np.asarray(constrained, dtype=np.int64)
    return np.concatenate([constrained, np.setdiff1d(np.arange(q, dtype=np.int64), constrained)])


def _event_host(what, arrays):
    if any(hasattr(a, "data_ptr") for a in arrays):
        raise ValueError(what + ": the scenarios are device tensors (device=True); copy them to the host first: this package "
                         "does no arithmetic in torch")


class EventScenarios:
    """What `event_samples` returns.
    draws [R, B, M, n]: scenarios in the components' own units, all inside the event; weights [R, B, n]: their importance weights;
    prob: the JointProbability of the event; ess [R, B]: (sum f)^2 / sum f^2, the effective sample size of each seed's n scenarios
    (NaN where every weight is 0); ok [M]: whether component m has a positive finite mass (false: its draws are NaN);
    uniforms [R, B, M, n]: the u behind the draws, draws = `quantiles(distrs, uniforms)` bit for bit (rows of given components:
    Fhat of the given value)."""

    def __init__(self, draws, weights, prob, ess, ok, uniforms):
        self.draws, self.weights, self.prob, self.ess, self.ok, self.uniforms = draws, weights, prob, ess, ok, uniforms

    def means(self):
        """(mean [B, M], stderr [B, M]) of E[X_m | event]: per seed the ratio sum f x / sum f, then the mean over the seeds and their
        sample standard deviation over sqrt(R) (NaN for one seed).  NaN for a box whose weights are all 0 in some seed"""
        _event_host("EventScenarios.means", (self.draws, self.weights))
        f = self.weights
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.einsum("rbn,rbmn->rbm", f, self.draws) / f.sum(axis=2)[:, :, None]
            R = ratio.shape[0]
            stderr = np.std(ratio, axis=0, ddof=1) / np.sqrt(R) if R > 1 else np.full(ratio.shape[1:], np.nan)
            return ratio.mean(axis=0), stderr

    def weighted_quantiles(self, probs):
        """[B, M, len(probs)]: the weighted quantiles of every component given the event from the scenarios of all seeds pooled:
        the smallest draw at which the cumulated normalised weight reaches p.  NaN for a box whose weights are all 0"""
        _event_host("EventScenarios.weighted_quantiles", (self.draws, self.weights))
        probs = np.atleast_1d(np.asarray(probs, dtype=np.float64)).reshape(-1)
        R, B, M, n = self.draws.shape
        out = np.full((B, M, probs.size), np.nan)
        valid = (probs >= 0) & (probs <= 1)
        for b in range(B):
            f = self.weights[:, b, :].reshape(-1)
            total = f.sum()
            if not total > 0:
                continue
            for m in range(M):
                x = self.draws[:, b, m, :].reshape(-1)
                if np.any(np.isnan(x)):
                    continue
                order = np.argsort(x, kind="stable")
                cum = np.cumsum(f[order]) / total
                at = np.minimum(np.searchsorted(cum, np.where(valid, probs, 0.0), side="left"), x.size - 1)
                out[b, m] = np.where(valid, x[order][at], np.nan)
        return out


_DRAWS_ORDER = "the draws entries keep one shared factor (`joint_probabilities(order=\"genz\")` reorders the probability)"


def event_samples(distrs, lower, upper, n, seeds, corr=None, factor=None, given=None, streams=None, first=0, qmc=True, device=False,
                  dof=None, mix_stream=None, mixing="plain", order="natural"):
    """Joint scenarios of ALL components GIVEN the event lower_m < X_m < upper_m for all m, under the marginals and the Gaussian
    copula of `joint_samples`, for B events and R seeds through `copula_box_draws` and ONE `quantiles` call: what the system
    looks like when the event of `joint_probabilities` happens.  Every scenario lies in the event and carries a weight; rejection
    (filtering `joint_samples`) keeps a fraction P of its draws, none at P = 1e-6.  Limits map to scores as in
    `joint_probabilities`; no component is dropped.  The components are drawn in the order: those that some box of the call
    constrains, ascending, then the others, ascending (the weights then vary least: `_event_order`), through the Cholesky factor
    of the correlation permuted so; the results come back in the caller's order.
    :param lower, upper: broadcast to [B, M] in the components' own units; +-inf, or a value at or beyond an end of the domain,
        does not constrain that side.  A given component must not be constrained
    :param corr, factor: as in `joint_probabilities`; exactly one of the two
    :param given: None, or the mapping of `conditional_samples`: the scenarios are conditional on these values too (the Schur
        factor, the conditional means as the shift); arrays [B] pair with the boxes (one box pairs with all sets).  The rows of
        given components hold the given values
    :param streams: one per chain position (there are M - len(given)); coordinate streams[i] draws the i-th component of the
        order above
    :param n, seeds, first, qmc: as in `copula_box_probabilities`
    :param device: draws, uniforms and weights are float64 torch device tensors; `means` and `weighted_quantiles` then raise
    :param dof, mix_stream: the STUDENT-T copula of `joint_samples(dof=...)`, as in `joint_probabilities`: the same chain order,
        `copula_box_draws(dof=...)` and one `quantiles` call on its u.  Under default streams `prob` is bit for bit that of
        `joint_probabilities(dof=...)` where no component is dropped there.  Not together with `given`: that is
        `conditional_event_samples`
    :param mixing: "plain" (default, bit for bit as before; ess / n of a deep event under a small dof is then tiny: the weights are
        carried by the few points with a rare mixing scale) or "conditioned" (dof only): the conditioned lead of `copula_box_draws`.
        The lead of each box is the constrained component with the smallest marginal probability (`lead_components`); it moves to
        the front of the chain order above, boxes are grouped by lead with one device call per group, and draws, uniforms and
        weights come back in the components' own order.  `prob` is bit for bit that of `joint_probabilities(mixing="conditioned")`
        where no component is dropped there.  Out of scope: `given` (raises) and reordering beyond the lead
    :param order: "natural" (the order above); "genz" raises: the draws entries keep one shared factor, so a per-box order cannot be
        expressed
    :return: EventScenarios"""
    _check_order("event_samples", order, _DRAWS_ORDER)
    return _event_samples("event_samples", False, distrs, lower, upper, n, seeds, corr, factor, given, streams, first, qmc, device, dof,
                          mix_stream, mixing)


def _lead_box_draws(corr, order, keep, t_lo, t_hi, n, seeds, streams, first, qmc, device, dof, mix_stream):
    """BoxDraws of `event_samples(mixing="conditioned")` with the rows of z and u in the chain order `order` (chain position ->
    component; the constrained components `keep` first): per box the lead (`lead_components` among `keep`; nothing constrained: the
    first of the order) moves to the front, boxes are grouped by lead, one `copula_box_draws` call per group on the correlation
    permuted so, and the rows go back to their chain positions"""
    B, q, R = t_lo.shape[0], order.size, seeds.size
    lead = lead_components(t_lo, t_hi, dof, keep)[0] if keep.size else np.full(B, order[0])
    z = u = w = None
    replicates = np.empty((R, B))
    for c, boxes in _lead_groups(lead):
        at = int(np.flatnonzero(order == c)[0])
        pos = np.concatenate([[at], np.delete(np.arange(q), at)])                            # the group's chain -> chain position
        comp = order[pos]
        low = correlation_factor(corr[np.ix_(comp, comp)])[0]
        box = copula_box_draws(low, t_lo[np.ix_(boxes, comp)], t_hi[np.ix_(boxes, comp)], n, [int(s) for s in seeds], streams=streams,
                               first=first, qmc=qmc, device=device, dof=dof, mix_stream=mix_stream, mixing="conditioned")
        replicates[:, boxes] = box.prob.replicates
        if z is None:
            new = (lambda shape: box.z.new_empty(shape)) if device else np.empty
            z, u, w = new((R, B, q, n)), new((R, B, q, n)), new((R, B, n))
        rows = boxes.tolist() if device else boxes
        w[:, rows] = box.weights
        for i, k in enumerate(pos):
            z[:, rows, int(k)] = box.z[:, :, i]
            u[:, rows, int(k)] = box.u[:, :, i]
    return BoxDraws(z, u, w, _joint_probability(replicates, n, seeds))


def _event_samples(what, conditional, distrs, lower, upper, n, seeds, corr, factor, given, streams, first, qmc, device, dof, mix_stream,
                   mixing="plain"):
    """the one body of `event_samples` and `conditional_event_samples` (conditional: the second one, where dof with given components
    goes through `conditional_box_draws`); the argument errors come in the order they have always had"""
    distrs = list(distrs)
    M = len(distrs)
    if M == 0:
        raise ValueError(what + ": no distributions")
    if conditional:
        dof = _conditional_dof(what, dof, mix_stream, given, M, "event_samples")
    else:
        dof = _box_dof(what, dof, mix_stream, given)
    lead = _check_mixing(what, mixing, dof, None, given)
    if (corr is None) == (factor is None):
        raise ValueError(what + ": exactly one of corr and factor must be given")
    n, seeds, first = _box_call_args(what, n, seeds, first)
    _common_quadrature(what, distrs)
    if factor is not None:
        fac = np.asarray(factor, dtype=np.float64)
        if fac.ndim != 2 or fac.shape[0] != M or fac.shape[1] < 1 or not np.all(np.isfinite(fac)):
            raise ValueError(what + ": the factor must be a finite [M, K] matrix with M = {} distributions".format(M))
        corr = fac @ fac.T
    corr = np.array(corr, dtype=np.float64)
    if corr.shape != (M, M):
        raise ValueError(what + ": corr must be [M, M] with M = {} distributions, got shape {}".format(M, corr.shape))
    if given is not None:
        observed, values, _ = _parse_given(what, given, M)
    else:
        observed, values = np.zeros(0, dtype=np.int64), np.zeros((0, 1))
    free = np.setdiff1d(np.arange(M, dtype=np.int64), observed)
    q = free.size
    lo, hi = _box_limits(what, lower, upper, M)
    B, Bg = lo.shape[0], values.shape[1]
    if Bg != 1 and B != 1 and Bg != B:
        raise ValueError(what + ": the arrays of given hold {} sets, there are {} boxes".format(Bg, B))
    if B == 1 and Bg > 1:
        lo, hi = np.repeat(lo, Bg, axis=0), np.repeat(hi, Bg, axis=0)
        B = Bg
    if q > _lib.BOX_PROB_MAX_M:
        raise ValueError(what + ": {} components exceed the cap of {}".format(q, _lib.BOX_PROB_MAX_M))
    z_lo, z_hi, keep, finish = _limit_scores(what, distrs, lo, hi)
    both = np.intersect1d(keep, observed)
    if both.size:
        raise ValueError(what + ": component {} is given and constrained by a limit: a given value is the condition, leave its "
                         "limits at -inf / +inf".format(int(both[0])))
    streams = _box_streams(what, streams, q + 1, qmc)
    if dof is not None:
        streams, mix_stream = _box_t_streams(what, dof, None, streams, mix_stream, q, qmc)
    finish()
    if dof is not None:
        z_lo, z_hi = t_scores(z_lo, dof), t_scores(z_hi, dof)
    # the chain: positions within the free components, constrained first
    perm = _event_order(np.searchsorted(free, keep), q)
    order = free[perm]                                                                       # chain position -> component
    if observed.size:
        cond = conditional_factor(corr, observed, return_observed=True) if dof is not None else None
        _, _, _, u_obs, (_, fc, _), mu, r = _conditioning(what, distrs, given, corr if cond is None else None, cond, dof)
        cov = fc @ fc.T
        low = np.linalg.cholesky(0.5 * (cov + cov.T)[np.ix_(perm, perm)])
        shift = np.ascontiguousarray(np.broadcast_to(mu[:, perm], (B, q)))
    else:
        low = correlation_factor(corr[np.ix_(order, order)])[0]
        u_obs, shift = None, None
    if lead:
        box = _lead_box_draws(corr, order, keep, z_lo, z_hi, n, seeds, streams, first, qmc, device, dof, mix_stream)
    elif observed.size and dof is not None:
        box = conditional_box_draws(low, z_lo[:, order], z_hi[:, order], n, [int(s) for s in seeds], dof, dof_mix=dof + observed.size,
                                    shift=shift, scale=np.broadcast_to(r, (B,)), streams=streams, first=first, qmc=qmc, device=device,
                                    mix_stream=mix_stream)
    else:
        box = copula_box_draws(low, z_lo[:, order], z_hi[:, order], n, [int(s) for s in seeds], shift=shift, streams=streams,
                               first=first, qmc=qmc, device=device, dof=dof, mix_stream=mix_stream)
    R = seeds.size
    # one quantiles call for all components: component order[i] takes the u of chain position i
    chain = [distrs[m] for m in order]
    if device:
        pts = [box.u[:, :, i, :].contiguous() for i in range(q)]
    else:
        pts = [np.ascontiguousarray(box.u[:, :, i, :]) for i in range(q)]
    xs, mass = _on_rule(chain, pts, True, what)
    ok = np.ones(M, dtype=bool)
    ok[order] = np.isfinite(mass) & (mass > 0)
    if device:
        import torch
        dev = box.u.device
        draws, uniforms = box.u.new_empty((R, B, M, n)), box.u.new_empty((R, B, M, n))
        for i, m in enumerate(order):
            draws[:, :, int(m), :] = xs[i]
            uniforms[:, :, int(m), :] = pts[i]
        if observed.size:
            vals = np.ascontiguousarray(np.broadcast_to(values.T, (B, observed.size)))
            uo = np.ascontiguousarray(np.broadcast_to(u_obs.T, (B, observed.size)))
            draws[:, :, observed.tolist(), :] = torch.from_numpy(vals).to(dev)[None, :, :, None]
            uniforms[:, :, observed.tolist(), :] = torch.from_numpy(uo).to(dev)[None, :, :, None]
        torch.cuda.current_stream(dev).synchronize()
        f = box.weights.cpu().numpy()
    else:
        draws, uniforms = np.empty((R, B, M, n)), np.empty((R, B, M, n))
        for i, m in enumerate(order):
            draws[:, :, m, :] = xs[i]
            uniforms[:, :, m, :] = pts[i]
        if observed.size:
            draws[:, :, observed, :] = np.broadcast_to(values.T, (B, observed.size))[None, :, :, None]
            uniforms[:, :, observed, :] = np.broadcast_to(u_obs.T, (B, observed.size))[None, :, :, None]
        f = box.weights
    with np.errstate(invalid="ignore", divide="ignore"):
        ess = f.sum(axis=2) ** 2 / (f * f).sum(axis=2)
    return EventScenarios(draws, box.weights, box.prob, ess, ok, uniforms)


# ---- aggregates of joint scenarios: functions of the components of one scenario column ------------------------------------------
Aggregates = collections.namedtuple("Aggregates", "rows names")
EventAggregates = collections.namedtuple("EventAggregates", "rows names weights")
RowStatistics = collections.namedtuple("RowStatistics", "mean var tail_prob tail_mean weight_sum n_used n_skipped")
_EXTREMES = {"max": _lib.AGG_MAX, "min": _lib.AGG_MIN, "argmax": _lib.AGG_ARGMAX, "argmin": _lib.AGG_ARGMIN}
_EXTRA_ORDER = (("max", _lib.AGG_MAX), ("min", _lib.AGG_MIN), ("count", _lib.AGG_COUNT), ("argmax", _lib.AGG_ARGMAX),
                ("argmin", _lib.AGG_ARGMIN))


def _aggregate_args(what, M, weights, lower, upper, members, extremes):
    """the checked arguments of mlmc_scenario_aggregates for M components, before anything touches the device:
    (W [A, M] or None, lower [M] or None, upper [M] or None, members uint8 [M] or None, extras bits, names of the Q rows)"""
    W = None
    if weights is not None:
        W = np.asarray(weights, dtype=np.float64)
        if W.ndim == 1:
            W = W[None, :]
        if W.ndim != 2 or W.shape[1] != M:
            raise ValueError("{}: weights must be [M] or [A, M] with M = {} components, got shape {}".format(
                what, M, np.shape(weights)))
        if not np.all(np.isfinite(W)):
            a, m = np.argwhere(~np.isfinite(W))[0]
            raise ValueError("{}: the weight of row {}, component {} is not finite".format(what, int(a), int(m)))
        W = np.ascontiguousarray(W)
    limits = []
    for name, lim in (("lower", lower), ("upper", upper)):
        if lim is not None:
            lim = np.asarray(lim, dtype=np.float64)
            try:
                lim = np.ascontiguousarray(np.broadcast_to(lim, (M,)))
            except ValueError:
                raise ValueError("{}: {} must broadcast to [M] with M = {} components, got shape {}".format(
                    what, name, M, lim.shape)) from None
            if np.any(np.isnan(lim)):
                raise ValueError("{}: the {} limit of component {} is NaN (use -inf / +inf for a side without a limit)".format(
                    what, name, int(np.flatnonzero(np.isnan(lim))[0])))
        limits.append(lim)
    lower, upper = limits
    if isinstance(extremes, str):
        extremes = (extremes,)
    extremes = tuple(extremes)
    extras = 0
    for name in extremes:
        if name not in _EXTREMES:
            raise ValueError("{}: extremes must be among 'max', 'min', 'argmax', 'argmin', got {!r}".format(what, name))
        extras |= _EXTREMES[name]
    if members is not None:
        mem = np.asarray(members)
        if mem.shape != (M,):
            raise ValueError("{}: members must be a mask [M] with M = {} components, got shape {}".format(what, M, mem.shape))
        members = np.ascontiguousarray(mem != 0, dtype=np.uint8)
        if extras and not members.any():
            raise ValueError(what + ": an extreme is requested and no component is a member")
    if lower is not None or upper is not None:
        extras |= _lib.AGG_COUNT
    A = 0 if W is None else W.shape[0]
    names = ["linear{}".format(a) for a in range(A)] + [name for name, bit in _EXTRA_ORDER if extras & bit]
    if not names:
        raise ValueError(what + ": nothing to compute: give weights, limits or extremes")
    return W, lower, upper, members, extras, names


def _aggregate_call(x, S, M, n, args, device):
    """mlmc_scenario_aggregates of x [S, M, n] (C-contiguous float64 NumPy array or device tensor) -> rows [S, Q, n] of its kind"""
    W, lower, upper, members, extras, names = args
    if hasattr(x, "data_ptr"):
        import torch
        out = torch.empty((S, len(names), n), dtype=torch.float64, device=x.device)
        torch.cuda.current_stream(x.device).synchronize()      # the library reads and writes on its own stream
        kind = _lib.DEVICE
    else:
        out, kind = np.empty((S, len(names), n)), _lib.HOST
    _lib.check(_lib.lib().mlmc_scenario_aggregates(_lib.ptr(x), S, M, n, n, _lib.ptr(W), 0 if W is None else W.shape[0], _lib.ptr(members),
                                                   _lib.ptr(lower), _lib.ptr(upper), extras, _lib.ptr(out), n, kind))
    return out


def _scenario_array(what, draws, device, lead):
    """draws as a C-contiguous float64 array of the kind the call works in (a device tensor for a device tensor or device=True), its
    shape checked: `lead` names the allowed leading axes"""
    if hasattr(draws, "data_ptr"):
        import torch
        if draws.dtype != torch.float64:
            raise ValueError(what + ": the draws must be float64, got {}".format(draws.dtype))
        x = draws.contiguous()
        if not x.is_cuda:
            x = x.numpy() if not device else x.cuda()
    else:
        x = np.ascontiguousarray(draws, dtype=np.float64)
        if device:
            import torch
            x = torch.from_numpy(x).cuda()
    if len(x.shape) not in lead:
        raise ValueError("{}: the array must have {} axes, got shape {}".format(
            what, " or ".join(str(k) for k in lead), tuple(x.shape)))
    return x


def scenario_aggregates(draws, weights=None, lower=None, upper=None, members=None, extremes=(), device=False):
    """Functions of the components of every scenario column, in ONE device call (mlmc_scenario_aggregates): the step from the
    scenarios of `joint_samples` / `conditional_samples` to the system-level quantities they exist for.  Per column j of a set:
      linear rows   sum_m W[a, m] x[m, j], the chain acc = acc + (W[a, m] * x[m, j]) over m ascending from +0.0 (two roundings per
                    step, no FMA): a total over a field, a portfolio;
      'max', 'argmax' (and 'min', 'argmin') over the components of `members`: np.argmax of the member subvector as a component
                    index (the first NaN if there is one) and x at that index: the worst component and which one it is;
      'count'       the number of components that have a finite limit and are NOT inside lower[m] < x < upper[m] (a NaN draw of
                    such a component counts): how many violate their limits at once; count == 0 is the box event of
                    `joint_probabilities`.  The row is present when lower or upper is given.
    A value depends on its own column, the weights, limits and members alone, so the result does not depend on n, on the sets
    or on how the caller blocks the columns, and host and device inputs give the same bits.
    :param draws: [M, n] or [S, M, n], a NumPy array or a float64 torch tensor (a device tensor is read in place)
    :param weights: None, [M] or [A, M], finite
    :param lower, upper: None or limits that broadcast to [M]; -inf / +inf: no limit on that side; NaN is an error
    :param members: None (all) or a mask [M]
    :param extremes: names among 'max', 'min', 'argmax', 'argmin'
    :param device: return a float64 torch device tensor also for a host input (a device input always does)
    :return: Aggregates(rows [Q, n] or [S, Q, n], names [Q]): the linear rows 'linear0' .. first, then 'max', 'min', 'count',
        'argmax', 'argmin' as far as requested; integer-valued rows are exact doubles"""
    what = "scenario_aggregates"
    x = _scenario_array(what, draws, device, (2, 3))
    M, n = int(x.shape[-2]), int(x.shape[-1])
    args = _aggregate_args(what, M, weights, lower, upper, members, extremes)
    S = 1 if len(x.shape) == 2 else int(x.shape[0])
    if S < 1:
        raise ValueError(what + ": no sets")
    out = _aggregate_call(x, S, M, n, args, device)
    return Aggregates(out[0] if len(x.shape) == 2 else out, args[-1])


def row_statistics(rows, f=None, thresholds=None, tail="upper"):
    """Weighted mean, variance, tail probability and tail mean of every row, through TWO calls of mlmc_rows_weighted_sums: the first
    gives the mean, the second sums about it, so the variance is a sum of terms of its own size.  With the weights f (None: ones)
    over the columns where neither the row nor f is NaN, d = y - mean1 of the first call:
        mean = mean1 + sum f d / sum f,   var = sum f d^2 / sum f - (sum f d / sum f)^2       (the weighted population variance)
        tail_prob[k] = sum f 1 / sum f,   tail_mean[k] = mean1 + sum f d 1 / sum f 1,   1 = (y >= t_k) for tail 'upper', (y <= t_k)
    for 'lower': with t the p-quantile of the row, tail_mean is the expected shortfall beyond it.  The sums are in a fixed order
    (include/mlmc_hip.h): a row's statistics do not depend on the other rows.  Negative or infinite weights are an error.
    :param rows: [..., n], a NumPy array or a float64 torch tensor (host or device)
    :param f: None or the weights [n] (brought to the memory of the rows)
    :param thresholds: None or [..., P] over the same leading axes (or [P]: the same thresholds for every row)
    :return: RowStatistics(mean [...], var [...], tail_prob [..., P], tail_mean [..., P], weight_sum [...], n_used [...],
        n_skipped [...]); a row without weight has NaN statistics, a tail without weight a NaN tail_mean"""
    what = "row_statistics"
    _check_tail_name(what, tail)
    y = _scenario_array(what, rows, False, tuple(range(1, 8)))
    lead, n = tuple(y.shape[:-1]), int(y.shape[-1])
    Rw = int(np.prod(lead, dtype=np.int64))
    on_device = hasattr(y, "data_ptr")
    if f is not None:
        if hasattr(f, "data_ptr"):
            f = f.detach().cpu().numpy()
        f = np.ascontiguousarray(f, dtype=np.float64)
        if f.shape != (n,):
            raise ValueError("{}: the weights must be [n] with n = {} columns, got shape {}".format(what, n, f.shape))
    if thresholds is None:
        t = np.zeros((Rw, 0))
    else:
        t = np.asarray(thresholds, dtype=np.float64)
        if t.ndim == 1:
            t = np.broadcast_to(t, lead + t.shape)
        if t.shape[:-1] != lead:
            raise ValueError("{}: thresholds must be [P] or {} + [P], got shape {}".format(what, list(lead), t.shape))
        if np.any(np.isnan(t)):
            raise ValueError(what + ": a threshold is NaN")
        t = np.ascontiguousarray(t.reshape(Rw, t.shape[-1]))
    P = t.shape[1]
    if on_device:
        import torch
        if f is not None:
            f = torch.from_numpy(f).to(y.device)
        torch.cuda.current_stream(y.device).synchronize()
    kind = _lib.DEVICE if on_device else _lib.HOST
    flag = _lib.TAIL_UPPER if tail == "upper" else _lib.TAIL_LOWER

    def call(c, thr):
        used, skipped = np.empty(Rw, dtype=np.int64), np.empty(Rw, dtype=np.int64)
        sums, tails = np.empty((Rw, 3)), np.empty((Rw, thr.shape[1], 2))
        _lib.check(_lib.lib().mlmc_rows_weighted_sums(_lib.ptr(y), Rw, n, n, _lib.ptr(f), _lib.ptr(c), _lib.ptr(thr), thr.shape[1], flag,
                                                      _lib.ptr(used), _lib.ptr(skipped), _lib.ptr(sums), _lib.ptr(tails), kind))
        return used, skipped, sums, tails

    with np.errstate(invalid="ignore", divide="ignore"):
        _, _, s1, _ = call(None, np.zeros((Rw, 0)))
        centre = s1[:, 1] / s1[:, 0]
        c = np.ascontiguousarray(np.where(np.isfinite(centre), centre, 0.0))
        used, skipped, s2, tails = call(c, t)
        sf = s2[:, 0]
        shift = s2[:, 1] / sf
        mean = np.where(np.isfinite(centre), c + shift, centre)
        var = s2[:, 2] / sf - shift * shift
        var = np.where(var < 0, 0.0, var)
        tail_prob = tails[:, :, 0] / sf[:, None]
        tail_mean = c[:, None] + tails[:, :, 1] / tails[:, :, 0]
    return RowStatistics(mean.reshape(lead), var.reshape(lead), tail_prob.reshape(lead + (P,)), tail_mean.reshape(lead + (P,)),
                         sf.reshape(lead), used.reshape(lead), skipped.reshape(lead))


def _check_tail_name(what, tail):
    if tail not in ("upper", "lower"):
        raise ValueError("{}: tail must be 'upper' or 'lower', got {!r}".format(what, tail))


def joint_aggregates(distrs, n, seed, weights=None, lower=None, upper=None, members=None, extremes=(), corr=None, factor=None,
                     given=None, streams=None, first=0, antithetic=False, qmc=False, block=2 ** 20, device=False, dof=None,
                     mix_stream=None):
    """`scenario_aggregates` of the scenarios of `joint_samples` (with `given`: of `conditional_samples`) WITHOUT the scenario
    matrix: the draw indices first .. first + n - 1 are walked in blocks of `block` columns, each block is drawn on the device,
    reduced there and dropped; only the aggregate rows are kept.  At M = 64 and n = 10^8 the matrix would be 51 GB, the result a
    few rows.  A draw depends on (seed, streams, j) alone and an aggregate on its own column alone, so the result is bit for bit
    `scenario_aggregates(joint_samples(distrs, n, ...), ...)` for EVERY block size.
    :param distrs, n, seed, corr, factor, streams, first, antithetic, qmc: as in `joint_samples`
    :param given: None, or the mapping of `conditional_samples` (arrays [B] give a leading axis B); `factor` then stands for the
        correlation factor @ factor.T
    :param weights, lower, upper, members, extremes: as in `scenario_aggregates`, over all M components (rows of given components
        hold the given values)
    :param block: columns per device block, >= 1 (with antithetic an even number)
    :param device: return the rows as a float64 torch device tensor
    :param dof, mix_stream: the Student-t copula of `joint_samples`; not together with `given`: that is `conditional_aggregates`
    :return: Aggregates(rows [Q, n], or [B, Q, n] for arrays in `given`; names)"""
    return _joint_aggregates("joint_aggregates", False, distrs, n, seed, weights, lower, upper, members, extremes, corr, factor, given,
                             streams, first, antithetic, qmc, block, device, dof, mix_stream)


def conditional_aggregates(distrs, n, seed, given, weights=None, lower=None, upper=None, members=None, extremes=(), corr=None,
                           factor=None, streams=None, first=0, antithetic=False, qmc=False, block=2 ** 20, device=False, dof=None,
                           mix_stream=None):
    """`joint_aggregates(given=...)`, the aggregates member of the conditional family, through the same body; with dof the block
    walk goes through `conditional_samples(dof=..., factor_info=the 4-tuple of conditional_factor)`, the conditional law of the
    Student-t copula.  Bit for bit `scenario_aggregates(conditional_samples(distrs, n, seed, given, ...), ...)` for every block size.
    :param given: the mapping of `conditional_samples` (required); the other arguments as in `joint_aggregates`
    :param dof, mix_stream: as in `conditional_samples`
    :return: Aggregates(rows [Q, n], or [B, Q, n] for arrays in `given`; names)"""
    return _joint_aggregates("conditional_aggregates", True, distrs, n, seed, weights, lower, upper, members, extremes, corr, factor,
                             given, streams, first, antithetic, qmc, block, device, dof, mix_stream)


def _joint_aggregates(what, conditional, distrs, n, seed, weights, lower, upper, members, extremes, corr, factor, given, streams, first,
                      antithetic, qmc, block, device, dof, mix_stream):
    """the one body of `joint_aggregates` and `conditional_aggregates` (conditional: the second one, which takes dof with given);
    the argument errors come in the order they have always had"""
    distrs = list(distrs)
    M = len(distrs)
    if M == 0:
        raise ValueError(what + ": no distributions")
    if conditional:
        dof = _conditional_dof(what, dof, mix_stream, given, M, "joint_aggregates")
    else:
        dof = _check_dof(what, dof)
        if dof is not None and given is not None:
            raise ValueError(what + ": dof together with given: this entry conditions under the Gaussian copula only; call "
                             "conditional_aggregates")
        if dof is None and mix_stream is not None:
            raise ValueError(what + ": mix_stream needs dof (the Gaussian copula has no mixing variable)")
    _sample_flags(what, antithetic, qmc)
    _check_seed(what, seed)
    if (corr is None) == (factor is None):
        raise ValueError(what + ": exactly one of corr and factor must be given")
    n = int(_per_distribution_int(what, "n", n, 1)[0])
    first = int(_per_distribution_int(what, "first", first, 1)[0])
    if isinstance(block, (bool, np.bool_)) or not isinstance(block, (int, np.integer)) or block < 1:
        raise ValueError(what + ": block must be a positive integer")
    if antithetic and (block % 2 or first % 2):
        raise ValueError(what + ": with antithetic, block and first must be even (a pair of draws shares its normals)")
    args = _aggregate_args(what, M, weights, lower, upper, members, extremes)
    lead = ()
    if given is not None:
        observed, values, scalar = _parse_given(what, given, M)
        if factor is not None:
            fac = np.asarray(factor, dtype=np.float64)
            if fac.ndim != 2 or fac.shape[0] != M or fac.shape[1] < 1 or not np.all(np.isfinite(fac)):
                raise ValueError(what + ": the factor must be a finite [M, K] matrix with M = {} distributions".format(M))
            corr = fac @ fac.T
        cond = conditional_factor(corr, observed, return_observed=dof is not None)
        lead = () if scalar else (values.shape[1],)
    elif corr is not None:
        factor = correlation_factor(corr)[0]
    import torch
    Q = len(args[-1])
    if device:
        rows = torch.empty(lead + (Q, n), dtype=torch.float64, device=torch.device("cuda", torch.cuda.current_device()))
    else:
        rows = np.empty(lead + (Q, n))
    for off in range(0, n, int(block)):
        nb = min(int(block), n - off)
        if given is None:
            x = joint_samples(distrs, nb, seed, factor=factor, streams=streams, first=first + off, antithetic=antithetic, device=True,
                              qmc=qmc, dof=dof, mix_stream=mix_stream)
        else:
            x = conditional_samples(distrs, nb, seed, given, factor_info=cond, streams=streams, first=first + off,
                                    antithetic=antithetic, device=True, qmc=qmc, dof=dof, mix_stream=mix_stream)
        S = 1 if x.dim() == 2 else int(x.shape[0])
        part = _aggregate_call(x, S, M, nb, args, True).reshape(lead + (Q, nb))
        if device:
            rows[..., off:off + nb] = part
        else:
            rows[..., off:off + nb] = part.cpu().numpy()
    if device:
        torch.cuda.current_stream(rows.device).synchronize()
    return Aggregates(rows, args[-1])


def event_aggregates(scen, weights=None, lower=None, upper=None, members=None, extremes=(), device=False):
    """`scenario_aggregates` of the scenarios of an `EventScenarios` (host or device arrays) in ONE device call: the aggregate rows
    of every seed and box next to the importance weights of the scenarios, ready for `row_statistics(rows[r, b], f=weights[r, b])`.
    :param scen: what `event_samples` returned
    :param weights, lower, upper, members, extremes, device: as in `scenario_aggregates` (`weights` are those of the linear rows)
    :return: EventAggregates(rows [R, B, Q, n], names [Q], weights [R, B, n])"""
    what = "event_aggregates"
    x = _scenario_array(what, scen.draws, device, (4,))
    R, B, M, n = (int(s) for s in x.shape)
    args = _aggregate_args(what, M, weights, lower, upper, members, extremes)
    if R * B < 1:
        raise ValueError(what + ": no scenarios")
    out = _aggregate_call(x.reshape(R * B, M, n), R * B, M, n, args, device)
    return EventAggregates(out.reshape(R, B, len(args[-1]), n), args[-1], scen.weights)


def _scores_problem_args(distrs, what):
    """the problem arguments of mlmc_density_scores_batch for a list of distributions, ready to be splatted into the call:
    (M, handles, r1, lam, sig, a, b, n_intervals, gauss_degree) as ctypes values, and the arrays that must outlive the call"""
    M = len(distrs)
    if M == 0:
        raise ValueError(what + ": no distributions")
    n_int, deg = _common_quadrature(what, distrs)
    handles, r1, lam, sig = _batch_problem_args(distrs)
    a, b = _domain_arrays(distrs)
    keep = (handles, r1, lam, sig, a, b)
    head = (M, C.cast(handles, C.c_void_p), _lib.ptr(r1), _lib.ptr(lam), _lib.ptr(sig), _lib.ptr(a), _lib.ptr(b), n_int, deg)
    return head, keep


def _scores_into(head, fine, coarse, n, ld_in, z_fine, z_coarse, ld_out, u_fine=None, u_coarse=None):
    """one call of mlmc_density_scores_batch on float64 device tensors (rows `ld_in` / `ld_out` apart, n columns used); the caller
    has synchronised the stream that produced the inputs"""
    _lib.check(_lib.lib().mlmc_density_scores_batch(*head, _lib.ptr(fine), _lib.ptr(coarse), int(n), int(ld_in), _lib.ptr(z_fine),
                                                    _lib.ptr(z_coarse), int(ld_out), _lib.ptr(u_fine), _lib.ptr(u_coarse), None))


def normal_scores(distrs, fine, coarse=None, device=False, return_uniforms=False):
    """Normal scores of stored samples under their fitted marginals through ONE device call (mlmc_density_scores_batch): row m of
    the result is z = Phi^-1(clamp(Fhat_m(x))) of row m of the input, Fhat_m of `cdfs_on_rule` (bit for bit its value), the clamp
    to [2^-53, 1 - 2^-53] of `joint_samples`.  A value that is NaN or outside the OPEN domain of its distribution gives NaN (the
    end points too): the densities were fitted to the in-domain samples alone, so the probability-integral transform is uniform
    on exactly those, and a NaN drops the sample in `quantity_estimate.component_covariance`.  So do all values of a distribution
    whose mass is not finite and positive or whose multipliers hold a NaN.  A score depends on (distribution, quadrature, value)
    alone.  The correlation of these scores is what a Gaussian copula over the marginals takes (`Estimate.estimate_score_correlation`).
    :param distrs: M distributions with multipliers, on one quadrature
    :param fine: [M, n] values, a NumPy array or a float64 torch device tensor; host input is uploaded once
    :param coarse: None or an array like `fine` (the coarse values of the same samples)
    :param device: return float64 torch device tensors
    :param return_uniforms: also return u = Fhat(x) (NaN where z is NaN)
    :return: z_fine, or (z_fine, z_coarse) with `coarse`; with return_uniforms the uniforms follow in the same order"""
    distrs = list(distrs)
    M = len(distrs)
    if M == 0:
        raise ValueError("normal_scores: no distributions")
    _common_quadrature("normal_scores", distrs)

    def checked(x, name):                                           # before anything touches the device
        if hasattr(x, "data_ptr"):
            if not x.is_cuda or str(x.dtype) != "torch.float64":
                raise ValueError("normal_scores: {} must be a NumPy array or a float64 device tensor".format(name))
        else:
            x = np.asarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[0] != M:
            raise ValueError("normal_scores: {} must be [M, n] with M = {} distributions, got shape {}".format(name, M, tuple(x.shape)))
        return x
    fine = checked(fine, "fine")
    coarse = None if coarse is None else checked(coarse, "coarse")
    if coarse is not None and tuple(coarse.shape) != tuple(fine.shape):
        raise ValueError("normal_scores: fine {} and coarse {} differ in shape".format(tuple(fine.shape), tuple(coarse.shape)))
    import torch
    head, _keep = _scores_problem_args(distrs, "normal_scores")                       # _keep: the arrays `head` points into
    dev = torch.device("cuda", torch.cuda.current_device())

    def on_device(x):
        return x.contiguous() if hasattr(x, "data_ptr") else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    f = on_device(fine)
    c = None if coarse is None else on_device(coarse)
    n = int(f.shape[1])
    outs = [torch.empty_like(f) for _ in range((1 if c is None else 2) * (2 if return_uniforms else 1))]
    torch.cuda.current_stream(f.device).synchronize()               # the library reads and writes on its own stream
    zf, zc = outs[0], (None if c is None else outs[1])
    uf = outs[-1 if c is None else -2] if return_uniforms else None
    uc = outs[-1] if return_uniforms and c is not None else None
    _scores_into(head, f, c, n, n, zf, zc, n, uf, uc)
    return_list = outs if device else [t.cpu().numpy() for t in outs]
    return return_list[0] if len(return_list) == 1 else tuple(return_list)


ConcordanceCounts = collections.namedtuple("ConcordanceCounts", "pair all kept")


def _concordance_limits(what, lower, upper, M):
    """lower, upper broadcast together to C-contiguous float64 [G, M] ([M] is one event), checked: no NaN, 1 <= G <= the cap"""
    lims = []
    for name, lim in (("lower", lower), ("upper", upper)):
        lim = np.asarray(lim, dtype=np.float64)
        if lim.ndim > 2:
            raise ValueError("{}: {} must broadcast to [G, M], got shape {}".format(what, name, lim.shape))
        if np.any(np.isnan(lim)):
            raise ValueError("{}: a {} limit is NaN (use -inf / +inf for a side without a limit)".format(what, name))
        lims.append(np.atleast_2d(lim))
    G = max(lims[0].shape[0], lims[1].shape[0])
    try:
        lims = [np.ascontiguousarray(np.broadcast_to(lim, (G, M))) for lim in lims]
    except ValueError:
        raise ValueError("{}: lower {} and upper {} must broadcast to [G, M] with M = {} components".format(
            what, np.shape(lower), np.shape(upper), M)) from None
    if not 1 <= G <= _lib.CONCORDANCE_MAX_G:
        raise ValueError("{}: {} events, between 1 and {} are supported per call".format(what, G, _lib.CONCORDANCE_MAX_G))
    return lims[0], lims[1]


def _concordance_into(fine, coarse, M, n, ld, lower, upper, pair, all_, kept, kernel_ms=None):
    """one call of mlmc_concordance_counts on float64 device tensors (rows `ld` apart, n columns used) and int64 device counters; the
    caller has synchronised the stream that produced them"""
    _lib.check(_lib.lib().mlmc_concordance_counts(_lib.ptr(fine), _lib.ptr(coarse), int(M), int(n), int(ld), int(lower.shape[0]),
                                                  _lib.ptr(lower), _lib.ptr(upper), _lib.ptr(pair), _lib.ptr(all_), _lib.ptr(kept),
                                                  None if kernel_ms is None else _lib.ptr(kernel_ms)))


def concordance_counts(fine, coarse=None, lower=-np.inf, upper=np.inf, pairs=True, device=False, out=None, kernel_ms=None):
    """How often the components lie inside box events, pair by pair and all at once, on bits in ONE device call
    (mlmc_concordance_counts).  Component m of a column is inside event g iff lower[g, m] < v < upper[g, m] (NaN never, a value on a
    limit not); a column with a NaN in any row of fine or coarse is dropped.  With e^f, e^c the inside indicators of a kept column
    (e^c = 0 without coarse), J_ab = e_a e_b and A = prod_m e_m:
      pair [G, 3, M, M] int64: sum J^f, sum J^c, sum [J^f != J^c] -- symmetric, the diagonal is the marginal count;
      all [G, 3] int64: the same three for A^f, A^c;      kept [1] int64: the kept columns.
    The level difference J^f - J^c is -1, 0 or 1, so its sum is pair[:, 0] - pair[:, 1] and the sum of its squares pair[:, 2]: the
    multilevel mean and variance of a joint frequency follow exactly (quantity_estimate.concordance_statistics).  All integer: the
    counts do not depend on how the columns are split across calls.
    :param fine: [M, n] values, a NumPy array or a float64 torch device tensor (rows may be a view with a row stride)
    :param coarse: None or an array like `fine`
    :param lower, upper: limits that broadcast to [G, M] ([M]: one event); -inf / +inf: no limit on that side; NaN is an error
    :param pairs: False: the `all` and `kept` counters alone (no bit matrix, no Gram); `pair` is None
    :param device: return int64 torch device tensors
    :param out: a ConcordanceCounts of int64 device tensors that the counts are ADDED to (it is returned: block after block)
    :param kernel_ms: None or a float64 NumPy array [2] that takes the HIP-event times of the two kernels
    :return: ConcordanceCounts(pair, all, kept)"""
    what = "concordance_counts"

    def checked(x, name):                                           # before anything touches the device
        if hasattr(x, "data_ptr"):
            if not x.is_cuda or str(x.dtype) != "torch.float64":
                raise ValueError("{}: {} must be a NumPy array or a float64 device tensor".format(what, name))
        else:
            x = np.asarray(x, dtype=np.float64)
        if len(x.shape) != 2:
            raise ValueError("{}: {} must be [M, n], got shape {}".format(what, name, tuple(x.shape)))
        return x
    fine = checked(fine, "fine")
    M, n = int(fine.shape[0]), int(fine.shape[1])
    if coarse is not None:
        coarse = checked(coarse, "coarse")
        if tuple(coarse.shape) != (M, n):
            raise ValueError("{}: fine {} and coarse {} differ in shape".format(what, tuple(fine.shape), tuple(coarse.shape)))
    if M > _lib.CONCORDANCE_MAX_M:
        raise ValueError("{}: {} components, at most {} are supported".format(what, M, _lib.CONCORDANCE_MAX_M))
    lower, upper = _concordance_limits(what, lower, upper, M)
    G = lower.shape[0]
    shapes = ((G, 3, M, M) if pairs else None, (G, 3), (1,))
    if out is not None:
        for name, t, shape in zip(ConcordanceCounts._fields, out, shapes):
            if shape is None and t is None:
                continue
            if shape is None or t is None or not getattr(t, "is_cuda", False) or str(t.dtype) != "torch.int64" \
                    or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("{}: out.{} must be a contiguous int64 device tensor of shape {}".format(what, name, shape))
    import torch
    dev = fine.device if hasattr(fine, "data_ptr") else torch.device("cuda", torch.cuda.current_device())

    def rows(x):
        """x on the device with unit column stride -> (tensor, row stride)"""
        if not hasattr(x, "data_ptr"):
            return torch.from_numpy(np.ascontiguousarray(x)).to(dev), n
        if n > 0 and M > 0 and (n == 1 or x.stride(1) == 1) and (M == 1 or x.stride(0) >= n):
            return x, (n if M == 1 else int(x.stride(0)))
        return x.contiguous(), n
    f, ld = rows(fine)
    c = None
    if coarse is not None:
        c, ld_c = rows(coarse)
        if ld_c != ld:
            f, c, ld = f.contiguous(), c.contiguous(), n
    if out is None:
        out = ConcordanceCounts(*[None if s is None else torch.zeros(s, dtype=torch.int64, device=dev) for s in shapes])
    torch.cuda.current_stream(dev).synchronize()                    # the library reads and writes on its own stream
    _concordance_into(f, c, M, n, ld, lower, upper, out.pair, out.all, out.kept, kernel_ms)
    if device:
        return out
    return ConcordanceCounts(*[None if t is None else t.cpu().numpy() for t in out])


_ORTHANT_RULE = {}


def bivariate_orthant(h, k, rho, nodes=64):
    """P(Z1 > h, Z2 > k) of standard normals with correlation rho, on the host, vectorised over arrays that broadcast: Plackett's
    formula  Phi(-h) Phi(-k) + (1 / 2 pi) int_0^{asin rho} exp(-(h^2 + k^2 - 2 h k sin t) / (2 cos^2 t)) dt  with a fixed
    Gauss-Legendre rule of `nodes` points.  The integrand is smooth on the closed interval for |rho| < 1 (64 nodes agree with
    scipy.stats.multivariate_normal.cdf to 1e-16 absolute up to rho = 0.999 at the levels 0.9 and 0.99); rho = 1 and rho = -1
    are taken as their limits Phi(-max(h, k)) and max(0, Phi(-k) - Phi(h)), not by the integral."""
    from scipy import special
    h, k, rho = np.broadcast_arrays(np.asarray(h, dtype=np.float64), np.asarray(k, dtype=np.float64), np.asarray(rho, dtype=np.float64))
    if np.any(np.isnan(rho)) or np.any(np.abs(rho) > 1.0):
        raise ValueError("bivariate_orthant: rho must lie in [-1, 1]")
    if nodes not in _ORTHANT_RULE:
        _ORTHANT_RULE[nodes] = np.polynomial.legendre.leggauss(int(nodes))
    x, w = _ORTHANT_RULE[nodes]
    inner = np.abs(rho) < 1.0
    half = 0.5 * np.arcsin(np.where(inner, rho, 0.0))[..., None]
    t = half * (1.0 + x)
    hh, kk = h[..., None], k[..., None]
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.exp(-(hh * hh + kk * kk - 2.0 * hh * kk * np.sin(t)) / (2.0 * np.cos(t) ** 2))
        integral = half[..., 0] * np.sum(w * f, axis=-1)
    out = special.ndtr(-h) * special.ndtr(-k) + integral / (2.0 * np.pi)
    out = np.where(rho >= 1.0, special.ndtr(-np.maximum(h, k)), out)
    out = np.where(rho <= -1.0, np.maximum(0.0, special.ndtr(-k) - special.ndtr(h)), out)
    return out if out.ndim else float(out)


_T_ORTHANT_RULE = {}


def _t_orthant_rule(nodes=96):
    """Gauss-Legendre panels in the probability of the mixing variable: (lower-tail probabilities, upper-tail probabilities,
    weights of both), with breaks at 1e-6, 1e-3, 0.05, 0.5 from either end"""
    if nodes not in _T_ORTHANT_RULE:
        x, w = np.polynomial.legendre.leggauss(int(nodes))
        breaks = (0.0, 1e-6, 1e-3, 0.05, 0.5)
        pp = np.concatenate([0.5 * (lo + hi) + 0.5 * (hi - lo) * x for lo, hi in zip(breaks[:-1], breaks[1:])])
        ww = np.concatenate([0.5 * (hi - lo) * w for lo, hi in zip(breaks[:-1], breaks[1:])])
        _T_ORTHANT_RULE[nodes] = (pp, ww)
    return _T_ORTHANT_RULE[nodes]


def bivariate_t_orthant(h, k, rho, dof):
    """P(T1 > h, T2 > k) of a bivariate Student-t pair with correlation parameter rho and `dof` degrees of freedom, on the host,
    vectorised over h, k, rho that broadcast (dof is one number).  (T1, T2) = (Z1, Z2) / sqrt(W) with W = chi2_dof / dof, so
        P = E_W[ bivariate_orthant(h sqrt(W), k sqrt(W), rho) ],
    taken by Gauss-Legendre panels in the probability of W (breaks at 1e-6, 1e-3, 0.05, 0.5 and their mirrors, 96 nodes each;
    W from the inverse incomplete gamma function of the nearer tail).  T1 and T2 share W, so they are dependent also at rho = 0:
    the value is then NOT the product of the marginals.  dof = np.inf returns `bivariate_orthant` itself; |rho| = 1 gives the
    limits, as there.  At h = k = 0 the value is 1/4 + asin(rho) / (2 pi) for every dof."""
    from scipy import special
    if isinstance(dof, (bool, np.bool_)) or np.ndim(dof) != 0 or not float(dof) > 0.0:
        raise ValueError("bivariate_t_orthant: dof must be one positive number (np.inf: the normal orthant)")
    nu = float(dof)
    if nu == np.inf:
        return bivariate_orthant(h, k, rho)
    h, k, rho = np.broadcast_arrays(np.asarray(h, dtype=np.float64), np.asarray(k, dtype=np.float64), np.asarray(rho, dtype=np.float64))
    if np.any(np.isnan(rho)) or np.any(np.abs(rho) > 1.0):
        raise ValueError("bivariate_t_orthant: rho must lie in [-1, 1]")
    pp, ww = _t_orthant_rule()
    a = 0.5 * nu
    root = np.sqrt(np.concatenate([special.gammaincinv(a, pp), special.gammainccinv(a, pp)]) / a)        # sqrt(W) at the nodes
    weights = np.concatenate([ww, ww])
    out = np.zeros(h.shape)
    flat_h, flat_k, flat_r, flat_o = h.reshape(-1), k.reshape(-1), rho.reshape(-1), out.reshape(-1)
    step = 256                                                       # points per slab: [step, nodes of W, nodes of the orthant]
    for i in range(0, flat_h.size, step):
        sl = slice(i, i + step)
        vals = bivariate_orthant(flat_h[sl, None] * root, flat_k[sl, None] * root, flat_r[sl, None])
        flat_o[sl] = np.sum(np.atleast_2d(vals) * weights, axis=-1)
    return out if out.ndim else float(out)


CopulaDofFit = collections.namedtuple("CopulaDofFit", "dof grid objective z")
COPULA_DOF_GRID = (2, 3, 4, 5, 6, 8, 10, 15, 20, 30, np.inf)


def _dof_grid(what, grid):
    """the candidate nu of a fit as a float64 array: finite values in [1, 64], np.inf for the Gaussian copula"""
    try:
        g = np.array([float(v) for v in grid], dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        g = np.array([np.nan])
    if g.size == 0 or not np.all((g == np.inf) | ((g >= 1.0) & (g <= 64.0))):
        raise ValueError(what + ": the grid must hold values in [1, 64] or np.inf")
    return g


def fit_copula_dof(prob, var, probs, corr, grid=COPULA_DOF_GRID):
    """The degrees of freedom of a Student-t copula from pair concordance frequencies, on the host: for every nu of `grid` the
    frequencies are held against the t orthant, and the nu with the smallest sum of squared z wins.  The frequencies do not
    depend on nu, so one pass over the samples serves the whole grid.
    :param prob, var: [G, M, M]: the estimate of P(U_a and U_b both beyond level p_g) and its variance
        (`Estimate.estimate_tail_dependence`, quantity_estimate.concordance_statistics)
    :param probs: [G] the levels p_g (an event u < 1 - p has the same model value as u > p, by symmetry)
    :param corr: [M, M] the copula's correlation matrix
    :param grid: candidate nu: finite values in [1, 64], np.inf for the Gaussian copula
    :return: CopulaDofFit(dof, grid, objective [len(grid)], z [len(grid), G, M, M]): z = (prob - model) / sqrt(var) with model =
        `bivariate_t_orthant` at h = k = T_nu^-1(p) and corr_ab, NaN on the diagonal and where var is not positive and finite;
        objective = the sum of z^2 over the pairs a < b and the events; dof = its argmin, a tie goes to the larger nu"""
    from scipy import special
    what = "fit_copula_dof"
    prob, var = np.asarray(prob, dtype=np.float64), np.asarray(var, dtype=np.float64)
    p = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    corr = np.asarray(corr, dtype=np.float64)
    if prob.ndim != 3 or prob.shape[1] != prob.shape[2] or var.shape != prob.shape:
        raise ValueError("{}: prob and var must be [G, M, M], got {} and {}".format(what, prob.shape, var.shape))
    G, M = prob.shape[0], prob.shape[1]
    if p.shape != (G,) or not np.all((p > 0.0) & (p < 1.0)):
        raise ValueError("{}: probs must be {} probability levels in (0, 1)".format(what, G))
    if corr.shape != (M, M) or not np.all(np.isfinite(corr)):
        raise ValueError("{}: corr must be a finite [{}, {}] matrix".format(what, M, M))
    g = _dof_grid(what, grid)
    rho = np.clip(corr, -1.0, 1.0)[None]
    z = np.full((g.size, G, M, M), np.nan)
    objective = np.empty(g.size)
    good = np.isfinite(var) & (var > 0.0) & np.triu(np.ones((M, M), dtype=bool), 1)[None]
    for i, nu in enumerate(g):
        h = (special.ndtri(p) if nu == np.inf else special.stdtrit(nu, p))[:, None, None]
        model = bivariate_t_orthant(h, h, rho, nu)
        with np.errstate(all="ignore"):
            zi = np.where(np.isfinite(var) & (var > 0.0), (prob - model) / np.sqrt(var), np.nan)
        zi[:, np.arange(M), np.arange(M)] = np.nan
        z[i] = zi
        objective[i] = float(np.sum(zi[good] ** 2))
    best = np.flatnonzero(objective == np.min(objective))
    dof = float(np.max(g[best])) if best.size else np.nan
    return CopulaDofFit(dof, g, objective, z)


CopulaLogDensity = collections.namedtuple("CopulaLogDensity", "fine coarse scores")
CopulaModels = collections.namedtuple("CopulaModels", "A logdet dof corr")


def _copula_models(what, corr, dofs, M=None):
    """the models of mlmc_copula_log_density: `dofs` one value or a sequence of G (np.inf: Gaussian), `corr` one correlation matrix
    for all or a sequence of G.  Each matrix goes through `correlation_factor` (the repaired matrix is the one that is inverted):
    A = F^-1 by a triangular solve, logdet = sum log F_ii.  -> CopulaModels(A [G, M, M], logdet [G], dof [G], corr [G, M, M])"""
    dof = _dof_grid(what, dofs if np.ndim(dofs) else [dofs])
    G = dof.size
    if G > _lib.COPULA_LIK_MAX_G:
        raise ValueError("{}: {} models, at most {} are supported per call".format(what, G, _lib.COPULA_LIK_MAX_G))
    try:
        c = np.asarray(corr, dtype=np.float64)
    except (TypeError, ValueError):
        c = None
    if c is None or c.ndim not in (2, 3) or c.shape[-1] != c.shape[-2] or (c.ndim == 3 and c.shape[0] != G):
        raise ValueError("{}: corr must be one correlation matrix [M, M] or one per model [{}, M, M]".format(what, G))
    if M is not None and c.shape[-1] != M:
        raise ValueError("{}: corr of shape {}, expected ({}, {})".format(what, c.shape[-2:], M, M))
    M = c.shape[-1]
    if not 1 <= M <= _lib.COPULA_LIK_MAX_M:
        raise ValueError("{}: {} components, between 1 and {} are supported".format(what, M, _lib.COPULA_LIK_MAX_M))
    mats = [c] if c.ndim == 2 else list(c)
    made = []
    for m in mats:
        F = correlation_factor(m)[0]
        made.append((scipy.linalg.solve_triangular(F, np.eye(M), lower=True), float(np.sum(np.log(np.diag(F)))), F @ F.T))
    if len(made) == 1:
        made = made * G
    return CopulaModels(np.ascontiguousarray(np.tril(np.stack([m[0] for m in made]))), np.array([m[1] for m in made]), dof,
                        np.stack([m[2] for m in made]))


def _copula_log_density_into(models, u_fine, u_coarse, n, ld, y_out=None, ll_fine=None, ll_coarse=None, ldo=0, sums=True, kind=None):
    """one call of mlmc_copula_log_density; the arrays are NumPy arrays or float64 device tensors of one kind (rows ld / ldo apart, n
    columns used); the caller has synchronised the stream that produced device inputs.  -> (kept, sums [3 G + G G]) or None"""
    G, M = models.A.shape[0], models.A.shape[1]
    kept = np.zeros(1, dtype=np.int64) if sums else None
    out = np.zeros(3 * G + G * G) if sums else None
    _lib.check(_lib.lib().mlmc_copula_log_density(M, G, _lib.ptr(models.A), _lib.ptr(models.logdet), _lib.ptr(models.dof),
                                                  _lib.ptr(u_fine), _lib.ptr(u_coarse), int(n), int(ld), _lib.ptr(y_out),
                                                  _lib.ptr(ll_fine), _lib.ptr(ll_coarse), int(ldo), _lib.ptr(kept), _lib.ptr(out),
                                                  _lib.mem_kind(u_fine) if kind is None else kind))
    return (int(kept[0]), out) if sums else None


def student_t_quantile(p, dof, device=False):
    """The quantile function of Student's t with `dof` degrees of freedom (a float in [1, 64]) on the device, elementwise
    (mlmc_student_t_quantile): the inverse of `student_t_cdf`, by Halley steps on the logarithm of its lower tail.
    quantile(1 - p) == -quantile(p) bit for bit for p > 1/2; -inf / +inf at 0 / 1, 0 at 1/2, NaN for NaN and outside [0, 1].
    :param p: a NumPy array or a float64 torch device tensor of any shape
    :param device: return a float64 torch device tensor"""
    return _t_elementwise("student_t_quantile", "mlmc_student_t_quantile", p, dof, device)


def copula_log_density(u, corr, dofs, u_coarse=None, device=False, return_scores=False):
    """The log density of Gaussian and Student-t copulas at columns of uniforms, for G models in ONE device call
    (mlmc_copula_log_density): l[g, j] = log c_g(u[:, j]).  A uniform is clamped to [2^-53, 1 - 2^-53]; a column with a NaN in any
    row (of `u_coarse` too, when given) is dropped: NaN in every output.  The mean of l over the samples' probability-integral
    transforms is the pseudo-likelihood of model g; `Estimate.estimate_copula_likelihood` forms it over the levels of a store.
    :param u: [M, n] uniforms, a NumPy array or a float64 torch device tensor
    :param corr: one correlation matrix [M, M] for all models, or a sequence of G; each goes through `correlation_factor`
    :param dofs: one value or a sequence of G: floats in [1, 64], np.inf for the Gaussian copula
    :param u_coarse: None or an array like `u` (the coarse values of the same samples)
    :param device: return float64 torch device tensors
    :param return_scores: also return the scores y [G, M, n] of `u`: normcdfinv(u) for a Gaussian model, the bits of
        `student_t_quantile(u, dof)` for a t model
    :return: l [G, n]; with `u_coarse` or `return_scores` CopulaLogDensity(fine, coarse, scores), None for what was not asked"""
    what = "copula_log_density"

    def checked(x, name):                                           # before anything touches the device
        if hasattr(x, "data_ptr"):
            if not x.is_cuda or str(x.dtype) != "torch.float64":
                raise ValueError("{}: {} must be a NumPy array or a float64 device tensor".format(what, name))
        else:
            x = np.asarray(x, dtype=np.float64)
        if len(x.shape) != 2 or x.shape[0] < 1:
            raise ValueError("{}: {} must be [M, n], got shape {}".format(what, name, tuple(x.shape)))
        return x
    u = checked(u, "u")
    M, n = int(u.shape[0]), int(u.shape[1])
    if u_coarse is not None:
        u_coarse = checked(u_coarse, "u_coarse")
        if tuple(u_coarse.shape) != (M, n) or hasattr(u_coarse, "data_ptr") != hasattr(u, "data_ptr"):
            raise ValueError("{}: u {} and u_coarse {} must be arrays of one kind and shape".format(what, tuple(u.shape),
                                                                                                   tuple(u_coarse.shape)))
    models = _copula_models(what, corr, dofs, M)
    G = models.dof.size
    on_device = hasattr(u, "data_ptr")
    if on_device:
        import torch
        u = u.contiguous()
        u_coarse = None if u_coarse is None else u_coarse.contiguous()
    else:
        u = np.ascontiguousarray(u)
        u_coarse = None if u_coarse is None else np.ascontiguousarray(u_coarse)
    shapes = ((G, M, n) if return_scores else None, (G, n), None if u_coarse is None else (G, n))
    if on_device:
        outs = [None if s is None else torch.empty(s, dtype=torch.float64, device=u.device) for s in shapes]
        torch.cuda.current_stream(u.device).synchronize()           # the library reads and writes on its own stream
    else:
        outs = [None if s is None else np.empty(s) for s in shapes]
    if n > 0:
        _copula_log_density_into(models, u, u_coarse, n, n, outs[0], outs[1], outs[2], n, sums=False)
    if on_device and not device:
        outs = [None if t is None else t.cpu().numpy() for t in outs]
    elif device and not on_device:
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        outs = [None if t is None else torch.from_numpy(t).to(dev) for t in outs]
    if u_coarse is None and not return_scores:
        return outs[1]
    return CopulaLogDensity(outs[1], outs[2], outs[0])


def likelihood_statistics(n, sd, sdd):
    """Level statistics of copula log densities from their sums (`quantity_estimate.component_copula_likelihood`): n [L] kept
    samples, sd [L, G] = sum_j d_g and sdd [L, G, G] = sum_j d_g d_h of the level differences d_g = l^f_g - l^c_g.  Through
    engine.level_stats: mean_l = s / n_l, var_l = (q - s^2 / n_l) / (n_l - 1), inf where n_l <= 1.
    -> dict(l_means, l_vars [L, G], loglik = sum_l mean_l, var = sum_l var_l / n_l [G], and the same for every paired difference
    d_g - d_h, whose sum of squares is sdd_gg + sdd_hh - 2 sdd_gh: delta_l_means, delta_l_vars [L, G, G], delta, delta_var [G, G])"""
    from .. import engine
    n = np.asarray(n, dtype=np.int64)
    sd = np.asarray(sd, dtype=np.float64)
    sdd = np.asarray(sdd, dtype=np.float64)
    if sd.ndim != 2 or n.shape != (sd.shape[0],) or sdd.shape != sd.shape + (sd.shape[1],):
        raise ValueError("likelihood_statistics: n [L], sd [L, G] and sdd [L, G, G] are expected, got {}, {} and {}".format(
            n.shape, sd.shape, sdd.shape))
    L, G = sd.shape
    nf = n.astype(np.float64)[:, None]
    diag = sdd[:, np.arange(G), np.arange(G)]
    l_means, l_vars = engine.level_stats(n, sd, diag)
    ds = (sd[:, :, None] - sd[:, None, :]).reshape(L, G * G)
    dq = (diag[:, :, None] + diag[:, None, :] - 2.0 * sdd).reshape(L, G * G)
    d_means, d_vars = engine.level_stats(n, ds, dq)
    with np.errstate(all="ignore"):
        var = np.sum(l_vars / nf, axis=0)
        d_var = np.sum(d_vars / nf, axis=0)
    return dict(l_means=l_means, l_vars=l_vars, loglik=np.sum(l_means, axis=0), var=var,
                delta_l_means=d_means.reshape(L, G, G), delta_l_vars=d_vars.reshape(L, G, G),
                delta=np.sum(d_means, axis=0).reshape(G, G), delta_var=d_var.reshape(G, G))


def joint_log_density(distrs, x, corr, dof=None):
    """The log of the joint density that the marginals `distrs` and a copula define, at the columns of x [M, n]:
    log c(Fhat_1(x_1), ..., Fhat_M(x_M)) + sum_m log rho_m(x_m), a host composition of `copula_log_density` with `cdfs_on_rule`
    and `densities`.  NaN where a component is NaN or outside the open domain of its distribution.
    :param corr: the copula's correlation matrix [M, M]
    :param dof: None or np.inf: the Gaussian copula; a float in [1, 64]: the Student-t copula
    :return: [n]"""
    what = "joint_log_density"
    distrs = list(distrs)
    M = len(distrs)
    if M == 0:
        raise ValueError(what + ": no distributions")
    nu = _check_dof(what, dof)
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] != M:
        raise ValueError("{}: x must be [M, n] with M = {} distributions, got shape {}".format(what, M, x.shape))
    models = _copula_models(what, corr, [np.inf if nu is None else nu], M)          # checks corr before any device call
    a, b = _domain_arrays(distrs)
    inside = (x > a[:, None]) & (x < b[:, None])
    mid = 0.5 * (a + b)
    safe = np.where(inside, x, mid[:, None])
    u = np.stack(cdfs_on_rule(distrs, list(safe)))
    rho = np.stack(densities(distrs, list(safe)))
    ll = copula_log_density(u, corr, models.dof)[0]
    with np.errstate(all="ignore"):
        out = ll + np.sum(np.log(rho), axis=0)
    return np.where(np.all(inside, axis=0), out, np.nan)


def _rvs(dist, n, seed, stream, first, antithetic, device, qmc=False):
    """the B = 1 call of `samples`"""
    return samples([dist], n, seed, streams=[stream], first=first, antithetic=antithetic, device=device, qmc=qmc)[0]


Divergences = collections.namedtuple("Divergences", "kl l2 tv hellinger mass_prior mass_posterior")


def divergences(priors, posteriors, intervals=None):
    """Distances between pairs of max-entropy densities through ONE device call (mlmc_density_divergences_batch): pair k compares
    the prior p = priors[k] with the posterior q = posteriors[k] (the roles of `KL_divergence(prior_density, posterior_density, a,
    b)`) on intervals[k] = (lo, hi), by default the intersection of the two domains.  On the distributions' common quadrature
    (n_intervals cells of _gauss_degree points over the interval)
        kl = int p log(p / q) - p + q,  l2 = sqrt(int (q - p)^2),  tv = 1/2 int |q - p|,  hellinger = sqrt(1/2 int (sqrt q - sqrt p)^2),
    with the densities as they are (not normalised; mass_prior and mass_posterior are their integrals over the interval).  The
    integrands are formed from p and the difference of the two exponents (include/mlmc_hip.h): no logarithm, no division, and a
    density against itself gives exactly 0.  A value is bit for bit the same for a pair alone or in any batch; an object that
    appears in many pairs is sent to the device once.  A density that is NaN on the interval gives NaN for the pair.
    :param priors, posteriors: equally long sequences of SimpleDistribution / Distribution objects with multipliers
    :param intervals: None, one (lo, hi) for all pairs, or one per pair; each inside both domains
    :return: Divergences(kl, l2, tv, hellinger, mass_prior, mass_posterior) of [P] arrays"""
    priors, posteriors = list(priors), list(posteriors)
    P = len(priors)
    if len(posteriors) != P:
        raise ValueError("divergences: {} priors for {} posteriors".format(P, len(posteriors)))
    if P == 0:
        return Divergences(*(np.empty(0) for _ in range(6)))
    index, distrs = {}, []
    for d in priors + posteriors:
        if id(d) not in index:
            index[id(d)] = len(distrs)
            distrs.append(d)
    n_int, deg = _common_quadrature("divergences", distrs)
    first = np.array([index[id(d)] for d in priors], dtype=np.int32)
    second = np.array([index[id(d)] for d in posteriors], dtype=np.int32)
    a, b = _domain_arrays(distrs)
    lo = hi = None                                                   # the library takes the intersections
    if intervals is None:
        empty = np.flatnonzero(~(np.maximum(a[first], a[second]) < np.minimum(b[first], b[second])))
        if empty.size:
            raise ValueError("divergences: pair {}: the two domains do not intersect".format(int(empty[0])))
    else:
        iv = np.asarray(intervals, dtype=np.float64)
        if iv.shape not in ((2,), (P, 2)):
            raise ValueError("divergences: intervals must be one (lo, hi) or one per pair, got shape {}".format(iv.shape))
        iv = np.broadcast_to(iv, (P, 2))
        lo, hi = np.ascontiguousarray(iv[:, 0]), np.ascontiguousarray(iv[:, 1])
    handles, r1, lam, sig = _batch_problem_args(distrs)
    out = np.empty((P, 6))
    _lib.check(_lib.lib().mlmc_density_divergences_batch(len(distrs), C.cast(handles, C.c_void_p), _lib.ptr(r1), _lib.ptr(lam),
                                                         _lib.ptr(sig), _lib.ptr(a), _lib.ptr(b), n_int, deg, P, _lib.ptr(first),
                                                         _lib.ptr(second), _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(out)))
    return Divergences(out[:, 0].copy(), np.sqrt(out[:, 1]), out[:, 2].copy(), np.sqrt(out[:, 3]), out[:, 4].copy(), out[:, 5].copy())


def _divergence(dist, prior, interval):
    """the P = 1 call of `divergences` with `dist` as the posterior: a Divergences of floats"""
    return Divergences(*(float(v[0]) for v in divergences([prior], [dist], None if interval is None else [tuple(interval)])))


DensityMoments = collections.namedtuple("DensityMoments", "moments entropy mass")
DensitySummary = collections.namedtuple("DensitySummary", "mean var skewness kurtosis entropy mass")


def _moment_problems(what, distrs, moments_fns, sizes):
    """(test moments objects [B], output counts [B]) of a `density_moments` call, checked before any device call"""
    B = len(distrs)
    if moments_fns is None:
        fns = [d.moments_fn for d in distrs]
        if sizes is None:
            sizes = [len(d.multipliers) for d in distrs]
    elif isinstance(moments_fns, moments_mod.Moments):
        fns = [moments_fns] * B
    else:
        fns = list(moments_fns)
        if len(fns) != B:
            raise ValueError("{}: {} moments objects for {} distributions".format(what, len(fns), B))
        if not all(isinstance(fn, moments_mod.Moments) for fn in fns):
            raise ValueError("{}: moments_fns must hold Moments objects".format(what))
    if sizes is None:
        sizes = [fn.size for fn in fns]
    elif np.isscalar(sizes):
        sizes = [sizes] * B
    sizes = list(sizes)
    if len(sizes) != B:
        raise ValueError("{}: {} sizes for {} distributions".format(what, len(sizes), B))
    seen = set()                                               # thousands of distributions usually share a few (object, size) pairs
    for i, (fn, k) in enumerate(zip(fns, sizes)):
        if (id(fn), id(k)) in seen:
            continue
        seen.add((id(fn), id(k)))
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= k <= fn.size:
            raise ValueError("{}: distribution {}: size must be an integer in 1..{}, got {!r}".format(what, i, fn.size, k))
        if getattr(fn, "_kind", None) not in (_lib.LEGENDRE, _lib.MONOMIAL, _lib.FOURIER, _lib.SPLINE):
            raise ValueError("{}: distribution {}: {} moments are not supported".format(what, i, type(fn).__name__))
    if distrs:
        _common_quadrature(what, distrs)
    return fns, np.array(sizes, dtype=np.int32)


def _raw_density_moments(what, distrs, moments_fns, sizes):
    """mlmc_density_moments_batch of a list of distributions: (raw moments [B, Kmax], counts [B], raw entropy column [B], mass [B])"""
    fns, k = _moment_problems(what, distrs, moments_fns, sizes)
    B = len(distrs)
    handles, r1, lam, sig = _batch_problem_args(distrs)
    a, b = _domain_arrays(distrs)
    tests = (C.c_void_p * B)(*[fn._basis_handle().value for fn in fns])
    out = np.empty((B, int(k.max())))
    mass, ent = np.empty(B), np.empty(B)
    _lib.check(_lib.lib().mlmc_density_moments_batch(B, C.cast(handles, C.c_void_p), _lib.ptr(r1), _lib.ptr(lam), _lib.ptr(sig),
                                                     _lib.ptr(a), _lib.ptr(b), int(distrs[0].n_intervals), int(distrs[0]._gauss_degree),
                                                     C.cast(tests, C.c_void_p), _lib.ptr(k), _lib.ptr(out), _lib.ptr(mass),
                                                     _lib.ptr(ent)))
    return out, k, ent, mass


def _normalized_entropy(ent, mass):
    """differential entropy of rho / T from the raw column -int rho log rho and the mass T"""
    with np.errstate(all="ignore"):
        return ent / mass + np.log(mass)


def density_moments(distrs, moments_fns=None, sizes=None, normalize=True):
    """Moments, differential entropy and mass of many max-entropy densities through ONE device call (mlmc_density_moments_batch):
    entry b of `moments` is int psi_j(x) rho_b(x) dx, j < sizes[b], for the moments object psi = moments_fns[b] -- any Legendre,
    Monomial, Fourier or Spline object or a TransformedMoments of one, with its own domain, unrelated to the basis of the density.
    A node of the quadrature outside a safe_eval object's domain makes that distribution's moments NaN.  On the distributions'
    common quadrature (include/mlmc_hip.h); a value is bit for bit the same for a distribution alone or in any batch.
    :param moments_fns: None: every distribution's own moments_fn at len(multipliers) -- the moments the solver has fitted, to
        compare with moment_means; one object for all; or one per distribution
    :param sizes: None: the full size of every object; one count for all; or one per distribution
    :param normalize: True: moments of rho / T and the entropy -int (rho / T) log(rho / T), T the mass; False: the raw
        int psi_j rho and -int rho log rho of the density as it is (the exponent clipped to +-200, as in `density`)
    :return: DensityMoments(moments: list of B arrays, entropy [B], mass [B])"""
    distrs = list(distrs)
    if not distrs:
        _moment_problems("density_moments", distrs, moments_fns, sizes)
        return DensityMoments([], np.empty(0), np.empty(0))
    out, k, ent, mass = _raw_density_moments("density_moments", distrs, moments_fns, sizes)
    if normalize:
        with np.errstate(all="ignore"):
            out = out / mass[:, None]
        ent = _normalized_entropy(ent, mass)
    return DensityMoments([row[:n] for row, n in zip(out, k.tolist())], ent, mass)        # rows of one array owned by the result


def _central_summary(r, scale, ref0, shift):
    """mean, variance, skewness and kurtosis (not excess) of x from the normalised raw moments r [B, 5] = E[t^k], k = 0 .. 4, of
    t = (x - shift) * scale + ref0: the exact raw-to-central formulas about t = 0, then x - shift = (t - ref0) / scale"""
    r = np.asarray(r, dtype=np.float64)
    r1, r2, r3, r4 = r[:, 1], r[:, 2], r[:, 3], r[:, 4]
    with np.errstate(all="ignore"):
        c2 = r2 - r1 * r1
        c3 = r3 - 3 * r1 * r2 + 2 * r1 ** 3
        c4 = r4 - 4 * r1 * r3 + 6 * r1 * r1 * r2 - 3 * r1 ** 4
        return (r1 - ref0) / scale + shift, c2 / scale ** 2, c3 / c2 ** 1.5, c4 / (c2 * c2)


def summaries(distrs):
    """Mean, variance, skewness, kurtosis (3 for a Gaussian), differential entropy and mass of many max-entropy densities from two
    device calls of `density_moments`' entry.  The first, with Monomial(2, domain), gives the mass and the centre m = a + W m_1 /
    m_0, W = b - a; the second takes the moments of t = (x - m) / W up to t^4 (a Monomial object whose reference domain is the
    domain shifted to the centre), so that the raw-to-central formulas subtract nothing of size: mu_1 ~ 0.  All on the
    distributions' common quadrature, of the normalised density rho / mass.
    :return: DensitySummary(mean, var, skewness, kurtosis, entropy, mass) of [B] arrays"""
    distrs = list(distrs)
    if not distrs:
        return DensitySummary(*(np.empty(0) for _ in range(6)))
    by_domain = {}                                             # one object (one device handle) per distinct domain
    first = [by_domain.setdefault(dom, moments_mod.Monomial(2, dom)) for dom in ((float(d.domain[0]), float(d.domain[1])) for d in distrs)]
    out, _, _, mass = _raw_density_moments("summaries", distrs, first, None)
    second = []
    for d, row in zip(distrs, out):
        a, b = float(d.domain[0]), float(d.domain[1])
        W = b - a
        with np.errstate(all="ignore"):
            m = a + W * (row[1] / row[0])
        if not a <= m <= b:                                    # a density without a mean (NaN multipliers): NaN statistics below
            m = 0.5 * (a + b)
        second.append(moments_mod.Monomial(5, (a, b), ref_domain=((a - m) / W, (b - m) / W), safe_eval=False))
    out, _, ent, mass = _raw_density_moments("summaries", distrs, second, None)
    with np.errstate(all="ignore"):
        r = out / mass[:, None]
    scale = np.array([fn._linear_scale for fn in second], dtype=np.float64)
    ref0 = np.array([fn.ref_domain[0] for fn in second], dtype=np.float64)
    shift = np.array([fn._linear_shift for fn in second], dtype=np.float64)
    mean, var, skew, kurt = _central_summary(r, scale, ref0, shift)
    return DensitySummary(mean, var, skew, kurt, _normalized_entropy(ent, mass), mass)


def _fitted_moments(dist):
    """the B = 1 call of `density_moments` with the distribution's own moments object"""
    return density_moments([dist]).moments[0]


def _summary(dist):
    """the B = 1 call of `summaries`: a DensitySummary of floats"""
    return DensitySummary(*(float(v[0]) for v in summaries([dist])))


def _entropy(dist):
    """the B = 1 call of `density_moments`: the differential entropy of the normalised density"""
    return float(density_moments([dist], sizes=1).entropy[0])


def estimate_densities_minimize(distrs, tol=1e-5, reg_param=0.01):
    """SimpleDistribution.estimate_density_minimize of every distribution in `distrs`, solved in ONE batched device call
    (mlmc_maxent_solve_batch: one workgroup per problem).  Each distribution gets exactly what its own call would do:
    initial multipliers, the normalisation fix, every OptimizeResult field.  All must share the quadrature
    (n_intervals, gauss degree).
    :return: list of OptimizeResult, one per distribution"""
    distrs = list(distrs)
    if not distrs:
        return []
    n_int, deg = _common_quadrature("estimate_densities_minimize", distrs)
    for d in distrs:
        d._initialize_params(d.approx_size, tol)
    solved = _solve_batch_on_device([d.moments_fn for d in distrs], [d.moment_means for d in distrs],
                                    [d._moment_errs for d in distrs], [d.domain for d in distrs],
                                    [d.multipliers for d in distrs], tol, max_it=100, n_intervals=n_int, gauss_degree=deg)
    return [d._finish_minimize(lam, grad, hess, info, tol) for d, (lam, grad, hess, info) in zip(distrs, solved)]


def _device_density(moments_fn, multipliers, errs, value):
    value = np.atleast_1d(np.asarray(value, dtype=np.float64))
    flat = np.ascontiguousarray(value.reshape(-1))
    out = np.empty_like(flat)
    lam = np.ascontiguousarray(multipliers, dtype=np.float64)
    sig = np.ascontiguousarray(errs[:len(lam)], dtype=np.float64)
    _lib.check(_lib.lib().mlmc_density_eval(moments_fn._basis_handle(), _lib.ptr(lam), _lib.ptr(sig), len(lam), _lib.ptr(flat),
                                            flat.size, _lib.ptr(out), _lib.HOST))
    return out.reshape(value.shape)


def _device_integrals(moments_fn, multipliers, errs, lo, hi, degree):
    lo = np.ascontiguousarray(lo, dtype=np.float64)
    hi = np.ascontiguousarray(hi, dtype=np.float64)
    out = np.empty_like(lo)
    lam = np.ascontiguousarray(multipliers, dtype=np.float64)
    sig = np.ascontiguousarray(errs[:len(lam)], dtype=np.float64)
    _lib.check(_lib.lib().mlmc_density_integrate(moments_fn._basis_handle(), _lib.ptr(lam), _lib.ptr(sig), len(lam), _lib.ptr(lo),
                                                 _lib.ptr(hi), lo.size, int(degree), _lib.ptr(out)))
    return out


def _cdf(dist, values):
    """Cumulative `n`-point Gauss-Legendre between successive values, as the reference does (:108-125) -- the
    intervals are independent, so they are integrated in one device launch and prefix-summed."""
    values = np.atleast_1d(values)
    lo_edges, hi_edges, idx = [], [], []
    last_x = dist.domain[0]
    for i, val in enumerate(values):
        if dist.domain[0] < val < dist.domain[1]:
            lo_edges.append(last_x)
            hi_edges.append(val)
            idx.append(i)
            last_x = val
    pieces = _device_integrals(dist.moments_fn, dist.multipliers, dist._moment_errs, lo_edges, hi_edges, 10) if idx else []
    cdf_y = np.empty(len(values))
    last_y, k = 0, 0
    for i, val in enumerate(values):
        if val <= dist.domain[0]:
            last_y = 0
        elif val >= dist.domain[1]:
            last_y = 1
        else:
            last_y = last_y + pieces[k]
            k += 1
        cdf_y[i] = last_y
    return cdf_y


class SimpleDistribution:
    """Maximum-entropy density for given moment means (reference: simple_distribution.py:9-327)."""

    def __init__(self, moments_obj, moment_data, domain=None, force_decay=(True, True), verbose=False):
        self.moments_fn = None
        if domain is None:
            domain = moments_obj.domain
        self.domain = domain
        self.decay_penalty = force_decay
        self._verbose = verbose
        if moment_data is not None:
            self.moment_means = moment_data[:, 0]
            self.moment_errs = np.sqrt(moment_data[:, 1])
        self.multipliers = None
        self.approx_size = len(self.moment_means)
        assert moments_obj.size >= self.approx_size
        self.moments_fn = moments_obj
        self._gauss_degree = 21
        self._penalty_coef = 0
        # composite Gauss-Legendre sub-intervals of the fixed device quadrature (the reference takes them from
        # QUADPACK's adaptive bisection; 64 x 21 points integrate the Legendre-61 cases of the reference tests to 1e-13)
        self.n_intervals = 64

    def estimate_density_minimize(self, tol=1e-5, reg_param=0.01):
        """:param tol: tolerance for the norm of the gradient (moment residuals divided by their std errors)
        :param reg_param: unused, as in the reference (:50)
        :return: OptimizeResult with x, success, nit, fun, jac, fun_norm, eigvals, solver_res"""
        self._initialize_params(self.approx_size, tol)
        lam, grad, hess, info = _solve_on_device(self.moments_fn, self.moment_means, self._moment_errs, self.domain, self.multipliers,
                                           tol, max_it=100, n_intervals=self.n_intervals, gauss_degree=self._gauss_degree)
        return self._finish_minimize(lam, grad, hess, info, tol)

    def _finish_minimize(self, lam, grad, hess, info, tol):
        """OptimizeResult and normalisation fix from a device solve (shared by the single and the batched solve)."""
        result = OptimizeResult()
        result.x = lam.copy()
        result.fun = info.fun
        result.nit = info.nit
        result.hess = hess
        result.success = bool(info.success)
        result.status = 0 if info.success else 1
        result.message = "Optimization terminated successfully." if info.success else "Maximum number of iterations has been exceeded."
        self.multipliers = lam
        jac_norm = info.grad_norm
        result.jac = grad
        if self._verbose:
            print("size: {} nits: {} tol: {:5.3g} res: {:5.3g} msg: {}".format(self.approx_size, result.nit, tol, jac_norm, result.message))
        with _SmallLapack():
            result.eigvals = np.linalg.eigvalsh(hess)
        result.solver_res = result.jac
        # normalisation fix exactly as the reference applies it (:81-86)
        moment_0 = info.moment0
        self.multipliers[0] -= np.log(moment_0)
        if result.success or jac_norm < tol:
            result.success = True
        result.nit = max(result.nit, 1)
        result.fun_norm = jac_norm
        return result

    def density(self, value):
        """exp(clip(-sum_i phi_i(x) lambda_i / sigma_i, +-200)) (reference: :96-105)"""
        return _device_density(self.moments_fn, self.multipliers, self._moment_errs, value)

    def cdf(self, values):
        return _cdf(self, values)

    def quantile(self, p):
        """Q(p): the x in the domain with Fhat(x) = p on this distribution's quadrature (see `quantiles`, of which this is the
        call with one distribution, hence bit for bit its value).  p: array-like, or a float64 torch device tensor (the result
        is a device tensor then, e.g. for inverse-transform sampling with the caller's own uniforms)."""
        return _quantile(self, p)

    def rvs(self, n, seed, stream=0, first=0, antithetic=False, device=False, qmc=False):
        """n seeded draws from this density: draws first .. first + n - 1 of stream `stream` under `seed` (see `samples`, of which
        this is the call with one distribution, hence bit for bit its values; `seed` is required).  qmc=True: coordinate `stream`
        (a dimension below 1024) of the scrambled Sobol' points first .. first + n - 1; n should be a power of two and `first` a
        multiple of it for the balance to hold, and the spread of the means of R seeds is the error bar."""
        return _rvs(self, n, seed, stream, first, antithetic, device, qmc)

    def expected_shortfall(self, p, tail="upper"):
        """Expected shortfall (CVaR) at level p on this distribution's quadrature: E[X | X >= Q(p)] for tail = "upper",
        E[X | X <= Q(p)] for "lower" (see `tail_means`, of which this is the call with one distribution, hence bit for bit its
        value).  p: as in `quantile`."""
        return _expected_shortfall(self, p, tail)

    def divergence(self, prior, interval=None):
        """KL, L2, total-variation and Hellinger distance of this density (the posterior) from `prior`, another distribution
        object on the same quadrature, over `interval` (default: the intersection of the two domains): `divergences` with one
        pair, hence bit for bit its values.  :return: Divergences of floats"""
        return _divergence(self, prior, interval)

    def fitted_moments(self):
        """The moments of the normalised density in this distribution's own moments object, int phi_i rho / int rho for
        i < len(multipliers): what the solver has fitted to moment_means (`density_moments` with one distribution, hence bit for
        bit its values)."""
        return _fitted_moments(self)

    def summary(self):
        """Mean, variance, skewness, kurtosis, differential entropy and mass of this density on its quadrature (`summaries` with
        one distribution, hence bit for bit its values).  :return: DensitySummary of floats"""
        return _summary(self)

    def entropy(self):
        """Differential entropy -int p log p of the normalised density p = rho / int rho on this distribution's quadrature."""
        return _entropy(self)

    def _initialize_params(self, size, tol=None):
        assert self.domain is not None
        assert tol is not None
        self._quad_tolerance = 1e-10
        self._moment_errs = self.moment_errs
        self.multipliers = np.zeros(size)
        self.multipliers[0] = -np.log(1 / (self.domain[1] - self.domain[0]))   # uniform density to start with
        self._quad_log = []

    def eval_moments(self, x):
        return self.moments_fn.eval_all(x, self.approx_size)

    def end_point_derivatives(self):
        """One-sided difference quotients of the moments at the domain end points (reference: :240-252)."""
        eps = 1e-10
        left = right = np.zeros((1, self.approx_size))
        if self.decay_penalty[0]:
            left = self.eval_moments(self.domain[0] + eps) - self.eval_moments(self.domain[0])
        if self.decay_penalty[1]:
            right = -self.eval_moments(self.domain[1]) + self.eval_moments(self.domain[1] - eps)
        return np.stack((left[0, :], right[0, :]), axis=0) / eps / self._moment_errs[None, :]


def _composite_gauss(domain, n_intervals, degree):
    pt, w = np.polynomial.legendre.leggauss(degree)
    edges = np.linspace(domain[0], domain[1], n_intervals + 1)
    a, b = edges[:-1, None], edges[1:, None]
    return ((pt[None, :] + 1) / 2 * (b - a) + a).ravel(), (w[None, :] * (b - a) / 2).ravel()


# ----------------------------------------------------------------------------------------------------------
# diagnostics with an externally given density (Python callable): host quadrature, device moment evaluation
# ----------------------------------------------------------------------------------------------------------
def compute_exact_moments(moments_fn, density, tol=1e-10):
    """(reference: :330-346)"""
    a, b = moments_fn.domain
    out = np.zeros(moments_fn.size)
    for i in range(moments_fn.size):
        out[i] = integrate.quad(lambda x, i=i: float(np.ravel(moments_fn.eval(i, x))[0]) * density(x), a, b, epsabs=tol)[0]
    return out


def compute_semiexact_moments(moments_fn, density, tol=1e-10, n_intervals=256):
    """Moments of a given density on a composite 21-point Gauss-Legendre rule (reference: :349-378, there on
    QUADPACK's sub-intervals)."""
    pts, w = _composite_gauss(moments_fn.domain, n_intervals, 21)
    return (density(pts) * w) @ moments_fn.eval_all(pts)


def compute_exact_cov(moments_fn, density, tol=1e-10):
    """(reference: :381-399)"""
    a, b = moments_fn.domain
    size = moments_fn.size
    out = np.zeros((size, size))
    for i in range(size):
        for j in range(i + 1):
            def fn(x, i=i, j=j):
                m = np.ravel(moments_fn.eval_all(x))
                return m[i] * m[j] * density(x)
            out[j][i] = out[i][j] = integrate.quad(fn, a, b, epsabs=tol)[0]
    return out


def compute_semiexact_cov(moments_fn, density, tol=1e-10, n_intervals=256):
    """(reference: :402-438)"""
    pts, w = _composite_gauss(moments_fn.domain, n_intervals, 21)
    phi = moments_fn.eval_all(pts)
    return (phi.T * (density(pts) * w)) @ phi


def KL_divergence(prior_density, posterior_density, a, b):
    """D_KL(P | Q) with the positivity-preserving integrand of the reference (:443-459)."""
    def integrand(x):
        p = prior_density(x)
        q = max(posterior_density(x), 1e-300)
        return p * np.log(p / q) - p + q
    return max(integrate.quad(integrand, a, b, epsabs=1e-10)[0], 1e-10)


def L2_distance(prior_density, posterior_density, a, b):
    """(reference: :462-464)"""
    return np.sqrt(integrate.quad(lambda x: (posterior_density(x) - prior_density(x)) ** 2, a, b))[0]


# ----------------------------------------------------------------------------------------------------------
# orthogonalisation of the moments w.r.t. the estimated covariance
# ----------------------------------------------------------------------------------------------------------
def best_fit_all(values, range_a, range_b):
    """Best linear fit over all index windows [a, b) from the given candidates (reference: :538-556)."""
    best, best_value = None, np.inf
    for a in range_a:
        for b in range_b:
            if 0 <= a and a + 2 < b < len(values):
                fit, res, _, _, _ = np.polyfit(np.arange(a, b), values[a:b], deg=1, full=1)
                value = res / ((b - a) ** 2)
                if value < best_value:
                    best, best_value = (a, b, fit), value
    return best


def best_p1_fit(values):
    """Longest window with a small linear-fit residual, found coarse-to-fine (reference: :560-579)."""
    if len(values) > 12:
        end = len(values) - len(values) % 2
        a, b, _ = best_p1_fit(np.mean(values[:end].reshape((-1, 2)), axis=1))
        a, b = 2 * a, 2 * b
        return best_fit_all(values, [a - 1, a, a + 1], [b - 1, b, b + 1])
    idx = range(len(values))
    return best_fit_all(values, idx, idx)


def detect_treshold_slope_change(values, log=True):
    """Index from which the (log) eigenvalue sequence follows one slope; smaller ones are extrapolated
    (reference: :584-609)."""
    values = np.array(values)
    first_pos = 0
    if log:
        first_pos = int(np.argmax(values > 0))
        values[first_pos:] = np.log(values[first_pos:])
    a, b, fit = best_p1_fit(values[first_pos:])
    poly = np.poly1d(fit)
    i_treshold = a + first_pos
    mod_vals = values.copy()
    mod_vals[:i_treshold] = poly(np.arange(-first_pos, a))
    if log:
        mod_vals = np.exp(mod_vals)
    return i_treshold, mod_vals


def construct_ortogonal_moments(moments, cov, tol=None):
    """Basis orthonormal w.r.t. the (centred) covariance estimated from samples (reference: :756-841).

    centring M = I - e0-column of cov; eigen-decomposition of M cov M^T; eigenvalues under the threshold are cut;
    L = RQ-factor of M^T V diag(1/sqrt(ev)) so that the new basis is a lower-triangular combination of the old one.
    (Small dense LAPACK on the host, like the reference; R <= 128.)
    :return: TransformedMoments, (eigenvalues, threshold, L)"""
    size = moments.size
    centre = np.eye(size)
    centre[:, 0] = -cov[:, 0]
    with _SmallLapack():
        centred = centre @ cov @ centre.T
        if size >= 96:
            # LAPACK's MRRR driver (dsyevr) takes 1.9 ms for a 128 x 128 matrix on one thread where NumPy's divide-and-conquer
            # call (dsyevd) takes 4.7 ms; below ~100 rows NumPy's is the faster one.  Only eigenvalues and the SPAN of the kept
            # eigenvectors enter L (the R factor of the RQ step absorbs their signs): the result is the same to rounding.
            ev, evec = scipy.linalg.eigh(centred, driver="evr")
        else:
            ev, evec = np.linalg.eigh(centred)
    if tol is None:
        _, fixed = detect_treshold_slope_change(ev, log=True)
        threshold = int(np.argmax(ev - fixed[0] > 0))
    else:
        threshold = int(np.argmax(ev > tol))
    ev_kept = np.flip(ev[threshold:], axis=0)
    evec_kept = np.flip(evec[:, threshold:], axis=1)
    icov_sqrt_t = centre.T @ evec_kept * (1 / np.sqrt(ev_kept))[None, :]
    with _SmallLapack():
        r_nm, _ = scipy.linalg.rq(icov_sqrt_t, mode='full')
    l_mn = r_nm.T
    if l_mn[0, 0] < 0:
        l_mn = -l_mn
    return moments_mod.TransformedMoments(moments, l_mn), (ev, threshold, l_mn)
