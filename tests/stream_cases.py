"""Stream-order cases: every public entry that can receive (or return) a CUDA tensor, with inputs that are STILL BEING WRITTEN
by torch's current stream when the entry is called.  Nothing here touches a device at import; torch and mlmc_amd are imported
inside the functions.

The library launches on one stream of its own (hipStreamNonBlocking, mlmc_init) that nothing orders behind torch's streams, so an
entry that hands a device tensor to it has to order the two itself (`_lib.order_after_torch`).  A test whose inputs are complete
when the entry is called cannot see a missing wait.  `late_like` makes inputs that are not: their memory holds NaN (integers: the
most negative value) until a copy from the settled tensors runs, and that copy sits on the current stream behind `CHAIN_OPS`
in-place adds over a `CHAIN_BYTES` scratch tensor.  An event recorded behind the copy says whether the producer has finished;
`Pending.check()`, called immediately before the entry under test, fails with "producer already finished" when it has.  An entry
that does not wait reads allocated, valid memory that holds NaN: no case can fault.

Sizing of the chain, measured on an MI355X with the package of the parent commit (tests/test_gpu_stream_order.py prints both
figures with `-s` and asserts the factor of ten): the chain of 1000 adds over 256 MiB takes 76.5 ms of GPU time by torch events;
the slowest inventoried entry on settled inputs, `conditional_aggregates` with dof (row conditional_aggregates_t), takes 3.54 ms of
host wall time (second call), 3.4 to 3.7 ms over four runs.  The chain outlasts it 21 times.
"""
import collections

import numpy as np

CHAIN_BYTES = 256 * 2 ** 20           # the scratch tensor of the producer chain
CHAIN_OPS = 1000                      # in-place adds over it in front of the late copy
# measured on the MI355X at the parent commit: GPU time of the chain and host wall time of the slowest inventoried entry on
# settled inputs; the chain has to take at least ten times as long
CHAIN_MEASURED = dict(chain_gpu_ms=76.5, slowest_entry_ms=3.54, slowest_entry="conditional_aggregates_t")

DOM = (-3.7190164854556804, 3.7190164854556804)
N_LEVEL = (3001, 2000, 1003)          # odd sizes, more than one block of every kernel, three levels
STEPS = (0.5, 0.07, 0.01)
M = 3                                 # components
R = 4                                 # moments
B = 8                                 # bootstrap replicates
SEED = 20240911

Row = collections.namedtuple("Row", "name covers build run flat prepare", defaults=(None,))
# build() -> (tensors, aux): the settled CUDA tensors the entry receives (possibly none) and everything else it needs
# prepare(aux) -> state: what has to exist BEFORE the producer is queued (None: the state is aux).  Creating an accumulator
#     destroys the one of the previous run, and freeing device memory waits for every stream, the producer's included
# run(tensors, state, pending) -> result; calls pending.check() immediately before the entry under test
# flat(result) -> list of NumPy arrays


def state_of(row, aux):
    return aux if row.prepare is None else row.prepare(aux)


# ---- the late-input helper ---------------------------------------------------------------------------------------------
class Pending:
    """The event behind a late producer.  check(): the validity condition of a case."""

    def __init__(self, event):
        self.event, self.checks = event, 0

    def check(self):
        self.checks += 1
        if self.event is not None and self.event.query():
            raise AssertionError("producer already finished: the entry would read settled inputs and the case proves nothing")


SETTLED = Pending(None)               # for the settled run of a row: nothing to check (its `checks` count is not used)

_scratch = {}


def _chain(torch, device, ops=None):
    """queue the producer chain on the current stream of `device`"""
    buf = _scratch.get(device)
    if buf is None:
        buf = _scratch[device] = torch.zeros(CHAIN_BYTES // 8, dtype=torch.float64, device=device)
    for _ in range(CHAIN_OPS if ops is None else ops):
        buf.add_(1.0)


def chain_gpu_ms(ops=None):
    """GPU time of the chain on the current stream, by torch events"""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    _chain(torch, dev, 2)                                     # the scratch tensor exists, the kernel is loaded
    torch.cuda.current_stream(dev).synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    _chain(torch, dev, ops)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def poison_of(dtype):
    import torch
    return float("nan") if dtype.is_floating_point else torch.iinfo(dtype).min


def late_like(src):
    """src: settled CUDA tensors (possibly none) -> (tensors of the same shape, dtype and stride, Pending).  The new tensors hold
    the poison value now -- gaps between strided rows too -- and the values of `src` once the current stream has worked off the
    chain.  With no tensors the current stream is simply busy, which is what an entry that writes its own device outputs with
    torch before the library fills the rest has to cope with."""
    import torch
    dev = src[0].device if src else torch.device("cuda", torch.cuda.current_device())
    out = []
    for s in src:
        extent = 1 + sum((n - 1) * st for n, st in zip(s.shape, s.stride())) if s.numel() else 0
        base = torch.full((max(extent, 1),), poison_of(s.dtype), dtype=s.dtype, device=s.device)
        out.append(base.as_strided(tuple(s.shape), tuple(s.stride())))
    torch.cuda.current_stream(dev).synchronize()             # the poison is in memory (a wait for a few fills, not for a producer)
    _chain(torch, dev)
    for d, s in zip(out, src):
        d.copy_(s)
    event = torch.cuda.Event()
    event.record()
    return out, Pending(event)


# ---- results -----------------------------------------------------------------------------------------------------------
def walk(obj, leaf):
    """leaf(x) for every tensor / array / number inside tuples, lists, dicts, namedtuples and plain objects"""
    if obj is None or isinstance(obj, (str, bytes)):
        return
    if isinstance(obj, np.ndarray) or hasattr(obj, "data_ptr") or np.isscalar(obj):
        leaf(obj)
    elif isinstance(obj, dict):
        for k in sorted(obj):
            walk(obj[k], leaf)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            walk(v, leaf)
    elif hasattr(obj, "__dict__"):
        walk(vars(obj), leaf)
    else:
        raise TypeError("stream_cases.walk: {}".format(type(obj)))


def cuda_tensors(obj):
    found = []
    walk(obj, lambda x: found.append(x) if hasattr(x, "data_ptr") and x.is_cuda else None)
    return found


def flat_any(result):
    """every array of a result, in order, on the host (the caller has waited for the library and for torch)"""
    out = []
    walk(result, lambda x: out.append(x.detach().cpu().numpy() if hasattr(x, "data_ptr") else np.asarray(x)))
    return out


def bits(a):
    """uint64 view of 8-byte items (NaN payloads and the sign of zero count), bytes otherwise"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize == 8 and a.dtype.kind in "fiu" else a.reshape(-1).view(np.uint8)


def same_bits(got, want):
    """two flat lists of arrays agree in number, dtype, shape and every bit"""
    if len(got) != len(want):
        return False
    return all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def first_difference(got, want):
    if len(got) != len(want):
        return "{} arrays, expected {}".format(len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        if g.dtype != w.dtype or g.shape != w.shape:
            return "array {}: {} {} against {} {}".format(i, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.flatnonzero(bits(g).reshape(-1) != bits(w).reshape(-1))
        if bad.size:
            k = int(bad[0])
            return "array {}: {} of {} items differ, first at {}: {!r} against {!r}".format(
                i, bad.size, g.size, k, g.reshape(-1)[k] if g.dtype.itemsize == 8 else None, w.reshape(-1)[k] if w.dtype.itemsize == 8 else None)
    return None


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def level_values(seed=SEED):
    """[(fine [M, n_l], coarse [M, n_l] | None)]: correlated pairs inside DOM mostly, NaNs in different rows, a few far outside"""
    rng = np.random.default_rng(seed)
    out = []
    for l, n in enumerate(N_LEVEL):
        f = rng.standard_normal((M, n)) * (1.0 + 0.1 * np.arange(M))[:, None] + 0.2 * np.arange(M)[:, None]
        c = f + STEPS[l] * rng.standard_normal((M, n)) if l else None
        f[0, 5::97] = np.nan
        f[M - 1, 3::251] = 40.0
        if c is not None:
            c[1, 7::131] = np.nan
        out.append((f, c))
    return out


def _level_tensors():
    """the level values as one flat tensor list [f0, f1, c1, f2, c2] and the chunk list built from such a list"""
    tensors = []
    for f, c in level_values():
        tensors.append(_cuda(f))
        if c is not None:
            tensors.append(_cuda(c))
    return tensors


def _chunks(tensors):
    """[(level, fine, coarse | None)] from the flat list"""
    out, k = [], 0
    for l in range(len(N_LEVEL)):
        f = tensors[k]
        c = tensors[k + 1] if l else None
        k += 2 if l else 1
        out.append((l, f, c))
    return out


def _legendre(size=R, dom=DOM):
    from mlmc_amd import Legendre
    return Legendre(size, dom)


def distributions(count=M):
    """`count` max-entropy densities with given multipliers on Legendre(3) over different domains: exp(-sum lam_k P_k), one hump"""
    from mlmc_amd import Legendre
    from mlmc_amd.tool import simple_distribution as sd
    out = []
    for m in range(count):
        dom = (-4.0 + 0.25 * m, 4.0 + 0.5 * m)
        d = sd.SimpleDistribution(Legendre(3, dom), np.stack([np.eye(3)[0], np.ones(3)], axis=1), domain=dom)
        d.multipliers = np.array([0.3, 0.2 * m - 0.1, 2.0 + 0.5 * m])
        d._moment_errs = np.ones(3)
        out.append(d)
    return out


def _corr():
    c = np.full((M, M), 0.4)
    np.fill_diagonal(c, 1.0)
    return c


def _values_in_domains(n, seed):
    """[M, n] values inside the domains of `distributions`, some NaN, some outside"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, n)) * 1.2
    x[1, 4::61] = np.nan
    x[2, 9::83] = 25.0
    return x


def _uniforms(n, seed):
    rng = np.random.default_rng(seed)
    u = rng.random((M, n))
    u[0, 3::71] = np.nan
    return u


# ---- rows: the accumulators --------------------------------------------------------------------------------------------
def _accum(mode):
    from mlmc_amd.engine import LevelAccumulator
    mode = {"moments": LevelAccumulator.MOMENTS, "cov": LevelAccumulator.COV}[mode]
    return LevelAccumulator(_legendre(), len(N_LEVEL), mode, n_comp=M)


def _xcov():
    from mlmc_amd.engine import ComponentCovAccumulator
    acc = ComponentCovAccumulator(M, len(N_LEVEL))
    acc.set_shift(0.2 * np.arange(M))
    return acc


def _run_push():
    def run(tensors, acc, pending):
        pending.check()
        for l, f, c in _chunks(tensors):
            acc.push(l, f, c)
        return acc.finalize(reduce=False)
    return run


def _run_estimate():
    def run(tensors, acc, pending):
        chunks = _chunks(tensors)
        pending.check()
        return acc.estimate(chunks, reduce=False)
    return run


def bootstrap_sizes():
    """[levels][B] picks per replicate"""
    rng = np.random.default_rng(SEED + 1)
    return [rng.integers(n // 2, n + 1, size=B) for n in N_LEVEL]


def _boot(kind):
    from mlmc_amd import engine
    if kind == "moments":
        return engine.BootstrapAccumulator(_legendre(), M, len(N_LEVEL), B)
    if kind == "component":
        return engine.ComponentBootstrapAccumulator([_legendre(R, (DOM[0] - 0.5 * m, DOM[1] + 0.25 * m)) for m in range(M)], R,
                                                    len(N_LEVEL), B)
    acc = engine.ComponentCovBootstrapAccumulator(M, len(N_LEVEL), B)
    acc.set_shift(0.1 * np.arange(M))
    return acc


def _run_bootstrap():
    def run(tensors, acc, pending):
        sizes = bootstrap_sizes()
        pending.check()
        for l, f, c in _chunks(tensors):
            acc.accum(l, f, c, sizes[l], SEED, l)
        return acc.finalize()
    return run


def _run_bootstrap_weights(tensors, aux, pending):
    from mlmc_amd import engine
    pending.check()
    return engine.bootstrap_weights(N_LEVEL[2], bootstrap_sizes()[2], SEED, stream=2, device=True)


# ---- rows: percentiles -------------------------------------------------------------------------------------------------
def _build_rows_view():
    """[M, n] rows inside a wider block: a view with a row stride of its own, read in place"""
    n = N_LEVEL[0]
    block = np.full((M, n + 5), 1e300)
    block[:, :n] = level_values()[0][0]
    return [_cuda(block)[:, :n]], None


def _run_percentiles(tensors, aux, pending):
    from mlmc_amd import engine
    pending.check()
    return engine.percentiles(tensors[0], [1.0, 50.0, 99.0])


def _run_row_percentiles(tensors, aux, pending):
    from mlmc_amd import engine
    pending.check()
    return engine.row_percentiles(tensors[0], [1.0, 50.0, 99.0])


# ---- rows: a storage of device samples ---------------------------------------------------------------------------------
def _spec():
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    return [QuantitySpec(name="q", unit="m", shape=(M, 1), times=[1], locations=['0'])]


def _build_pairs():
    """per level [M, n, 3]: the pairs are the view [:, :, :2], which set_level_samples has to copy"""
    out = []
    for f, c in level_values():
        block = np.zeros(f.shape + (3,))
        block[:, :, 0] = f
        block[:, :, 1] = 0.0 if c is None else c
        block[:, :, 2] = 1e300
        out.append(_cuda(block)[:, :, :2])
    return out, None


def _device_storage(tensors, pending):
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.sample_storage import DeviceMemory
    qe.device_cache_clear()
    st = DeviceMemory()
    st.save_global_data(result_format=_spec(), level_parameters=[[s] for s in STEPS])
    st.save_n_ops([(l, (float(n) / STEPS[l], n)) for l, n in enumerate(N_LEVEL)])
    pending.check()
    for l, pairs in enumerate(tensors):
        st.set_level_samples(l, pairs)
    return st, make_root_quantity(st, _spec())['q'][1]['0']


def _run_storage_mean(tensors, aux, pending):
    from mlmc_amd.quantity import quantity_estimate as qe
    st, q = _device_storage(tensors, pending)
    tree = (q[1, 0] - 0.25) * q[0, 0]                         # a device program over two stored rows (DevicePlan.evaluate)
    out = []
    for quantity in (tree, q):
        r = qe.estimate_mean(qe.moments(quantity, _legendre(R, (-20.0, 20.0))))
        out.append((r.mean, r.var, r.l_means, r.l_vars, r.n_samples))
    qe.device_cache_clear()
    return out


def _run_storage_domains(tensors, aux, pending):
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    st, q = _device_storage(tensors, pending)
    out = Estimate.estimate_domains(q, st)
    qe.device_cache_clear()
    return out


def _run_storage_diagnostics(tensors, aux, pending):
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    st, q = _device_storage(tensors, pending)
    n, n_rm, stats = qe.level_diagnostics(q)
    d = Estimate(q, st, _legendre()).estimate_level_diagnostics()
    qe.device_cache_clear()
    return n, n_rm, stats, d


def _synth_storage(aux):
    """a generated storage with resident rows that has just been told to grow"""
    from mlmc_amd import _lib
    from mlmc_amd.quantity.quantity_spec import ChunkSpec
    from mlmc_amd.sim.synth_device import SynthDeviceStorage
    st = SynthDeviceStorage([[s] for s in STEPS], [900, 700, 500])
    for l in range(3):
        st.device_row(ChunkSpec(level_id=l), 3)
    _lib.check(_lib.lib().mlmc_synchronize())
    st.set_n_samples([n for n in N_LEVEL])
    return st


def _run_synth_storage(tensors, st, pending):
    """the resident rows are copied into a larger tensor by torch, then extended by the library"""
    from mlmc_amd import _lib
    from mlmc_amd.quantity.quantity_spec import ChunkSpec
    pending.check()
    rows = [st.device_row(ChunkSpec(level_id=l), 3) for l in range(3)]
    _lib.check(_lib.lib().mlmc_synchronize())                 # generated rows are the library's until it is waited for
    return [r.clone() for r in rows]


# ---- rows: tool.simple_distribution ------------------------------------------------------------------------------------
def _sd():
    from mlmc_amd.tool import simple_distribution as sd
    return sd


def _build_points(kind):
    def build():
        rng = np.random.default_rng(SEED + 2)
        if kind == "values":
            pts = [rng.uniform(-5.0, 6.0, size=(37, 11)) for _ in range(M)]
            pts[1][3, 4] = np.nan
        else:
            pts = [rng.random((37, 11)) for _ in range(M)]
            pts[2][0, 0], pts[2][0, 1], pts[0][5, 5] = 0.0, 1.0, np.nan
        return [_cuda(p) for p in pts], distributions()
    return build


def _run_on_rule(name):
    def run(tensors, aux, pending):
        pending.check()
        return getattr(_sd(), name)(aux, list(tensors))
    return run


def _build_t_argument(uniform):
    def build():
        rng = np.random.default_rng(SEED + 3)
        x = rng.random((41, 73)) if uniform else 3.0 * rng.standard_normal((41, 73))
        x[7, 7] = np.nan
        return [_cuda(x)], None
    return build


def _run_t(name, dof):
    def run(tensors, aux, pending):
        pending.check()
        return getattr(_sd(), name)(tensors[0], dof, device=True)
    return run


def _build_distrs():
    return [], distributions()


GIVEN = {1: np.array([-0.5, 0.3, 1.1])}


def _run_conditional_samples(dof):
    def run(tensors, aux, pending):
        pending.check()
        return _sd().conditional_samples(aux, 2048 + 5, SEED, GIVEN, corr=_corr(), device=True, return_uniforms=True, dof=dof)
    return run


def _run_joint_samples(tensors, aux, pending):
    pending.check()
    return _sd().joint_samples(aux, 2048 + 5, SEED, corr=_corr(), device=True, return_uniforms=True, return_normals=True)


def _run_samples(tensors, aux, pending):
    pending.check()
    return _sd().samples(aux, 2048 + 5, SEED, device=True, return_uniforms=True)


def _box():
    lower = np.array([[-1.0, -np.inf, -0.5], [0.2, -0.3, -np.inf]])
    upper = np.array([[1.5, 0.8, np.inf], [np.inf, 1.0, 2.0]])
    return lower, upper


def _run_event_samples(conditional, dof):
    def run(tensors, aux, pending):
        lower, upper = _box()
        pending.check()
        if conditional:
            lower, upper = lower.copy(), upper.copy()
            lower[:, 1], upper[:, 1] = -np.inf, np.inf
            return _sd().conditional_event_samples(aux, lower, upper, {1: 0.4}, 1024, [SEED, SEED + 1], corr=_corr(), device=True, dof=dof)
        return _sd().event_samples(aux, lower, upper, 1024, [SEED, SEED + 1], corr=_corr(), device=True, dof=dof)
    return run


def _factor():
    return np.linalg.cholesky(_corr())


def _run_box(name, dof):
    def run(tensors, aux, pending):
        lower, upper = _box()
        sd = _sd()
        pending.check()
        if name == "copula_box_probabilities":
            return sd.copula_box_probabilities(_factor(), lower, upper, 1024, [SEED, SEED + 1], return_integrand=True, device=True, dof=dof)
        if name == "copula_box_draws":
            return sd.copula_box_draws(_factor(), lower, upper, 1024, [SEED, SEED + 1], device=True, dof=dof)
        if name == "conditional_box_probabilities":
            return sd.conditional_box_probabilities(_factor(), lower, upper, 1024, [SEED, SEED + 1], dof, dof_mix=dof + 1, shift=0.1,
                                                    scale=1.2, return_integrand=True, device=True)
        return sd.conditional_box_draws(_factor(), lower, upper, 1024, [SEED, SEED + 1], dof, dof_mix=dof + 1, shift=0.1, scale=1.2,
                                        device=True)
    return run


def _aggregate_kw():
    return dict(weights=np.array([[1.0, 1.0, 1.0], [0.5, -2.0, 0.25]]), lower=[-1.0, -np.inf, -0.5], upper=[1.5, 0.8, np.inf],
                members=[1, 0, 1], extremes=("max", "min", "argmax", "argmin"))


def _build_scenarios():
    rng = np.random.default_rng(SEED + 4)
    x = rng.standard_normal((2, M, 3001))
    x[1, 2, 11::97] = np.nan
    return [_cuda(x)], None


def _run_scenario_aggregates(tensors, aux, pending):
    pending.check()
    return _sd().scenario_aggregates(tensors[0], **_aggregate_kw())


def _build_event():
    rng = np.random.default_rng(SEED + 5)
    return [_cuda(rng.standard_normal((2, 2, M, 1003))), _cuda(rng.random((2, 2, 1003)))], None


def _run_event_aggregates(tensors, aux, pending):
    sd = _sd()
    scen = sd.EventScenarios(tensors[0], tensors[1], None, None, None, None)
    pending.check()
    out = sd.event_aggregates(scen, **_aggregate_kw())
    return out.rows, out.names, out.weights


def _build_statistics():
    rng = np.random.default_rng(SEED + 6)
    rows = rng.standard_normal((2, 3, 3001))
    rows[1, 1, 5::89] = np.nan
    f = rng.random(3001)
    f[17] = np.nan
    return [_cuda(rows), _cuda(f)], None


def _run_row_statistics(tensors, aux, pending):
    pending.check()
    return _sd().row_statistics(tensors[0], f=tensors[1], thresholds=[-0.5, 1.0])


def _run_joint_aggregates(conditional, dof):
    def run(tensors, aux, pending):
        sd = _sd()
        pending.check()
        if conditional:
            return sd.conditional_aggregates(aux, 2048 + 5, SEED, GIVEN, corr=_corr(), block=1000, device=True, dof=dof, **_aggregate_kw())
        return sd.joint_aggregates(aux, 2048 + 5, SEED, corr=_corr(), block=1000, device=True, dof=dof, **_aggregate_kw())
    return run


def _build_pair_values():
    return [_cuda(_values_in_domains(3001, SEED + 7)), _cuda(_values_in_domains(3001, SEED + 8))], distributions()


def _run_normal_scores(tensors, aux, pending):
    pending.check()
    return _sd().normal_scores(aux, tensors[0], tensors[1], device=True, return_uniforms=True)


def _build_concordance():
    """fine / coarse rows inside wider blocks (read in place with their row stride) and the counters of an earlier block"""
    import torch
    n = 3001
    tensors = []
    for seed in (SEED + 9, SEED + 10):
        block = np.full((M, n + 3), 1e300)
        block[:, :n] = _values_in_domains(n, seed)
        tensors.append(_cuda(block)[:, :n])
    G = 2
    for shape in ((G, 3, M, M), (G, 3), (1,)):
        tensors.append(torch.arange(int(np.prod(shape)), dtype=torch.int64).reshape(shape).cuda())
    return tensors, None


def _concordance_limits():
    return np.array([[-1.0, -0.5, -np.inf], [0.0, -np.inf, 0.3]]), np.array([[1.0, np.inf, 0.9], [np.inf, 1.5, 2.0]])


def _run_concordance(with_out):
    def run(tensors, aux, pending):
        sd = _sd()
        lower, upper = _concordance_limits()
        out = sd.ConcordanceCounts(*[t.clone() for t in tensors[2:]]) if with_out else None    # the counts are ADDED: a copy per run
        pending.check()
        return tuple(sd.concordance_counts(tensors[0], tensors[1], lower, upper, device=True, out=out))
    return run


def _build_uniforms():
    return [_cuda(_uniforms(3001, SEED + 11)), _cuda(_uniforms(3001, SEED + 12))], None


def _run_copula_log_density(tensors, aux, pending):
    pending.check()
    out = _sd().copula_log_density(tensors[0], _corr(), [np.inf, 4.0, 9.5], u_coarse=tensors[1], device=True, return_scores=True)
    return tuple(out)


def _build_none():
    return [], None


def _levels():
    return _level_tensors(), None


_E = "mlmc_amd.engine:"
_S = "mlmc_amd.tool.simple_distribution:"
_Q = "mlmc_amd.quantity.quantity_estimate:"

INVENTORY = [
    Row("accum_push_moments", [_E + "LevelAccumulator.push", _E + "LevelAccumulator.finalize"], _levels, _run_push(), flat_any, lambda aux: _accum("moments")),
    Row("accum_push_cov", [_E + "LevelAccumulator.push", _E + "LevelAccumulator.finalize"], _levels, _run_push(), flat_any, lambda aux: _accum("cov")),
    Row("accum_estimate_moments", [_E + "LevelAccumulator.estimate"], _levels, _run_estimate(), flat_any, lambda aux: _accum("moments")),
    Row("accum_estimate_cov", [_E + "LevelAccumulator.estimate"], _levels, _run_estimate(), flat_any, lambda aux: _accum("cov")),
    Row("xcov_push", [_E + "LevelAccumulator.push", _E + "ComponentCovAccumulator.set_shift"], _levels, _run_push(), flat_any, lambda aux: _xcov()),
    Row("xcov_estimate", [_E + "LevelAccumulator.estimate", _E + "ComponentCovAccumulator.set_shift"], _levels, _run_estimate(), flat_any, lambda aux: _xcov()),
    Row("bootstrap_moments", [_E + "BootstrapAccumulator.accum"], _levels, _run_bootstrap(), flat_any, lambda aux: _boot("moments")),
    Row("bootstrap_component", [_E + "BootstrapAccumulator.accum"], _levels, _run_bootstrap(), flat_any, lambda aux: _boot("component")),
    Row("bootstrap_xcov", [_E + "BootstrapAccumulator.accum", _E + "ComponentCovBootstrapAccumulator.set_shift"], _levels,
        _run_bootstrap(), flat_any, lambda aux: _boot("xcov")),
    Row("bootstrap_weights", [_E + "bootstrap_weights"], _build_none, _run_bootstrap_weights, flat_any),
    Row("percentiles", [_E + "percentiles"], _build_rows_view, _run_percentiles, flat_any),
    Row("row_percentiles", [_E + "row_percentiles"], _build_rows_view, _run_row_percentiles, flat_any),
    Row("device_memory_estimate_mean", ["mlmc_amd.quantity.lowering:DevicePlan.evaluate"], _build_pairs, _run_storage_mean, flat_any),
    Row("device_memory_estimate_domains", [_E + "row_percentiles"], _build_pairs, _run_storage_domains, flat_any),
    Row("device_memory_level_diagnostics", [_Q + "_component_chunks", _Q + "_component_entry", _Q + "_device_rows"], _build_pairs,
        _run_storage_diagnostics, flat_any),
    Row("synth_storage_grown_rows", ["mlmc_amd.sim.synth_device:generate_rows"], _build_none, _run_synth_storage, flat_any, _synth_storage),
    Row("cdfs_on_rule", [_S + "_on_rule"], _build_points("values"), _run_on_rule("cdfs_on_rule"), flat_any),
    Row("quantiles", [_S + "_on_rule"], _build_points("probs"), _run_on_rule("quantiles"), flat_any),
    Row("tail_means", [_S + "_on_rule"], _build_points("probs"), _run_on_rule("tail_means"), flat_any),
    Row("student_t_cdf", [_S + "_t_elementwise"], _build_t_argument(False), _run_t("student_t_cdf", 4.5), flat_any),
    Row("student_t_quantile", [_S + "_t_elementwise"], _build_t_argument(True), _run_t("student_t_quantile", 4.5), flat_any),
    Row("chi2_mixing_scale", [_S + "_t_elementwise"], _build_t_argument(True), _run_t("chi2_mixing_scale", 4.5), flat_any),
    Row("conditional_mixing_scale", [_S + "_t_elementwise"], _build_t_argument(True), _run_t("conditional_mixing_scale", 70.5), flat_any),
    Row("samples", [_S + "_samples_flat"], _build_distrs, _run_samples, flat_any),
    Row("joint_samples", [_S + "joint_samples"], _build_distrs, _run_joint_samples, flat_any),
    Row("conditional_samples", [_S + "conditional_samples"], _build_distrs, _run_conditional_samples(None), flat_any),
    Row("conditional_samples_t", [_S + "conditional_samples"], _build_distrs, _run_conditional_samples(5.0), flat_any),
    Row("copula_box_probabilities", [_S + "copula_box_probabilities"], _build_none, _run_box("copula_box_probabilities", None), flat_any),
    Row("copula_box_probabilities_t", [_S + "copula_box_probabilities"], _build_none, _run_box("copula_box_probabilities", 5.0), flat_any),
    Row("copula_box_draws", [_S + "copula_box_draws"], _build_none, _run_box("copula_box_draws", None), flat_any),
    Row("copula_box_draws_t", [_S + "copula_box_draws"], _build_none, _run_box("copula_box_draws", 5.0), flat_any),
    Row("conditional_box_probabilities", [_S + "conditional_box_probabilities"], _build_none, _run_box("conditional_box_probabilities", 5.0),
        flat_any),
    Row("conditional_box_draws", [_S + "conditional_box_draws"], _build_none, _run_box("conditional_box_draws", 5.0), flat_any),
    Row("event_samples", [_S + "copula_box_draws", _S + "_on_rule"], _build_distrs, _run_event_samples(False, None), flat_any),
    Row("event_samples_t", [_S + "copula_box_draws", _S + "_on_rule"], _build_distrs, _run_event_samples(False, 5.0), flat_any),
    Row("conditional_event_samples", [_S + "copula_box_draws", _S + "_on_rule"], _build_distrs, _run_event_samples(True, None), flat_any),
    Row("conditional_event_samples_t", [_S + "conditional_box_draws", _S + "_on_rule"], _build_distrs, _run_event_samples(True, 5.0),
        flat_any),
    Row("scenario_aggregates", [_S + "_aggregate_call"], _build_scenarios, _run_scenario_aggregates, flat_any),
    Row("event_aggregates", [_S + "_aggregate_call"], _build_event, _run_event_aggregates, flat_any),
    Row("row_statistics", [_S + "row_statistics"], _build_statistics, _run_row_statistics, flat_any),
    Row("joint_aggregates", [_S + "_aggregate_call", _S + "joint_samples"], _build_distrs, _run_joint_aggregates(False, None), flat_any),
    Row("joint_aggregates_t", [_S + "_aggregate_call", _S + "joint_samples"], _build_distrs, _run_joint_aggregates(False, 5.0), flat_any),
    Row("conditional_aggregates", [_S + "_aggregate_call", _S + "conditional_samples"], _build_distrs, _run_joint_aggregates(True, None),
        flat_any),
    Row("conditional_aggregates_t", [_S + "_aggregate_call", _S + "conditional_samples"], _build_distrs, _run_joint_aggregates(True, 5.0),
        flat_any),
    Row("normal_scores", [_S + "_scores_into"], _build_pair_values, _run_normal_scores, flat_any),
    Row("concordance_counts", [_S + "_concordance_into"], _build_concordance, _run_concordance(False), flat_any),
    Row("concordance_counts_added", [_S + "_concordance_into"], _build_concordance, _run_concordance(True), flat_any),
    Row("copula_log_density", [_S + "_copula_log_density_into"], _build_uniforms, _run_copula_log_density, flat_any),
]

# the rows by name, once more: a row that disappears from INVENTORY is missed here (tests/test_stream_inventory_cpu.py)
REQUIRED_ROWS = (
    "accum_push_moments", "accum_push_cov", "accum_estimate_moments", "accum_estimate_cov", "xcov_push", "xcov_estimate",
    "bootstrap_moments", "bootstrap_component", "bootstrap_xcov", "bootstrap_weights", "percentiles", "row_percentiles",
    "device_memory_estimate_mean", "device_memory_estimate_domains", "device_memory_level_diagnostics", "synth_storage_grown_rows",
    "cdfs_on_rule", "quantiles", "tail_means", "student_t_cdf", "student_t_quantile", "chi2_mixing_scale", "conditional_mixing_scale",
    "samples", "joint_samples", "conditional_samples", "conditional_samples_t", "copula_box_probabilities",
    "copula_box_probabilities_t", "copula_box_draws", "copula_box_draws_t", "conditional_box_probabilities", "conditional_box_draws",
    "event_samples", "event_samples_t", "conditional_event_samples", "conditional_event_samples_t", "scenario_aggregates",
    "event_aggregates", "row_statistics", "joint_aggregates", "joint_aggregates_t", "conditional_aggregates",
    "conditional_aggregates_t", "normal_scores", "concordance_counts", "concordance_counts_added", "copula_log_density",
)

# rows whose result tensors belong to the LIBRARY's stream by their documented contract until mlmc_synchronize: the outputs test
# (read at once with torch) leaves them out; the row itself waits before it reads
LIBRARY_STREAM_OUTPUTS = ("synth_storage_grown_rows",)

_HOST_ONLY = "passes NumPy arrays only (problem tables, host outputs); the parser cannot prove it from the source"
EXEMPT = {
    "mlmc_amd._lib:ptr": "the accessor itself: it turns what it is given into a pointer and calls nothing",
    _E + "LevelAccumulator._finalize_distributed": "needs an initialised process group (tests/test_dist_gloo.py and the RCCL test of "
                                                   "test_gpu_api.py); the packed tensor is the library's own output buffer",
    _Q + "_subsample_on_device": "reads the resident rows that _chunk_for_device returned, which the storage or the library's own stream "
                                 "produced; a host chunk is uploaded and waited for in the function; its draws come from a global generator",
    _S + "_device_integrals": _HOST_ONLY,
    _S + "_raw_density_moments": _HOST_ONLY,
    _S + "_scores_problem_args": _HOST_ONLY,
    _S + "_solve_batch_on_device": _HOST_ONLY,
    _S + "cdfs": _HOST_ONLY,
    _S + "densities": _HOST_ONLY,
    _S + "divergences": _HOST_ONLY,
    _S + "sobol_table": _HOST_ONLY,
}
