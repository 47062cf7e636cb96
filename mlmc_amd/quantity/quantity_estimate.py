"""MLMC mean / variance estimation of quantities (reference interface: mlmc/quantity/quantity_estimate.py:6-156).

`estimate_mean`, `moments`, `moment`, `covariance`, `mask_nan_samples`, `cache_clear` keep the reference's names,
arguments, return type (`QuantityMean`) and error behaviour.  What differs is where the work happens: for every
storage chunk the raw fine / coarse arrays [M, n] go to the MI355X once; the moment functions, the NaN /
out-of-domain mask, the level differences and the sums of quantity_estimate.py:43-65 are fused into the HIP
accumulation kernels (mlmc_amd/csrc/moments.hip, cov.hip).  Nothing of shape [M*R, n, 2] or [M*R*R, n, 2] is
ever materialised.
"""
import collections
import contextlib
import functools
import itertools
import os
import threading

import numpy as np

from . import lowering
from . import quantity as qmod
from . import quantity_types as qt
from .. import engine
from .. import linearize


def mask_nan_samples(chunk):
    """Drop samples with a NaN in fine or coarse (reference: quantity_estimate.py:6-14).  Host helper kept for API
    compatibility; the estimators apply the same rule on the device."""
    mask = np.any(np.isnan(chunk), axis=0).any(axis=1)
    return chunk[..., ~mask, :], np.count_nonzero(mask)


def cache_clear():
    qmod.cache_clear()


class _MomentsNode(qmod.Quantity):
    """Quantity node 'moments of x'; evaluated lazily on the device when somebody asks for its samples, fused into
    the accumulation kernel when it is the root of an estimate."""

    def __init__(self, quantity, moments_fn, at_bottom, qtype):
        self._moments_fn = moments_fn
        self._at_bottom = at_bottom
        super().__init__(quantity_type=qtype, input_quantities=[quantity], operation=self._eval)

    def _eval(self, x):
        mom = self._moments_fn.eval_all(x)                      # [M, n, 2, R] (device evaluated)
        mom = mom.transpose((0, 3, 1, 2)) if self._at_bottom else mom.transpose((3, 0, 1, 2))
        return mom.reshape((int(np.prod(mom.shape[:-2])), mom.shape[-2], mom.shape[-1]))


class _CovarianceNode(qmod.Quantity):
    def __init__(self, quantity, moments_fn, at_bottom, qtype):
        self._moments_fn = moments_fn
        self._at_bottom = at_bottom
        super().__init__(quantity_type=qtype, input_quantities=[quantity], operation=self._eval)

    def _eval(self, x):
        # The reference materialises [M*R*R, n, 2] doubles here (quantity_estimate.py:131-147).  On this path the
        # outer products only ever exist inside the MFMA covariance kernel; there is no host fallback.
        raise NotImplementedError("samples of a covariance quantity are not materialised; use estimate_mean(covariance(...))")


class _ComponentCovNode(qmod.Quantity):
    """Quantity node 'covariance between the components of x' (component_covariance).  Like _CovarianceNode its samples are
    never materialised: estimate_mean sends the raw component values to the component-covariance accumulator."""
    _at_bottom = True

    def __init__(self, quantity, shift, qtype, scores=None):
        self._shift = shift
        self._scores = scores
        self._moments_fn = None
        super().__init__(quantity_type=qtype, input_quantities=[quantity], operation=self._eval)

    def _eval(self, x):
        raise NotImplementedError("samples of a component covariance are not materialised; use "
                                  "estimate_mean(component_covariance(...))")


# Bound of the score workspace of component_covariance(scores=...): the fine and coarse scores of one column block (the
# counterpart of Q_JOINT_BYTES in mlmc_amd/csrc/density.hip).  A level is processed in blocks of a FIXED number of columns, so
# that the same input gives the same bits; MLMC_SCORE_BLOCK_COLUMNS in the environment, read per estimate, overrides the
# number of columns (a test aid: the sums then differ by the rounding of another order of addition).
SCORE_BLOCK_BYTES = 64 << 20


def score_block_columns(n_comp):
    """columns of a score block for `n_comp` components (plus the row of ones): whole tiles of 64 within SCORE_BLOCK_BYTES"""
    env = int(os.environ.get("MLMC_SCORE_BLOCK_COLUMNS", "0") or 0)
    if env > 0:
        return env
    return max(64, SCORE_BLOCK_BYTES // (2 * 8 * (int(n_comp) + 1)) // 64 * 64)


def component_covariance(quantity, shift=None, scores=None):
    """Quantity of qtype ArrayType((M, M)) whose estimate_mean is the multilevel covariance between the M scalar components
    of `quantity` (row order: as Estimate.construct_densities documents -- the qtype flattened from the outside in).

    scores = a list of M distributions with multipliers (tool.simple_distribution, one quadrature): the components enter not as
    they are but as their NORMAL SCORES z_m = Phi^-1(Fhat_m(x_m)) under these marginals (mlmc_density_scores_batch), followed by
    a row of ones, so the qtype is ArrayType((M + 1, M + 1)): entry (i, j), i, j < M, is the multilevel second moment of the
    scores, row / column M their multilevel means and entry (M, M) is 1.  estimate_mean transforms each (fine, coarse) pair on the
    device right before the push, in column blocks of score_block_columns(M) columns; the scores never leave the device and every
    stored chunk is read once.  A value that is NaN or outside its marginal's open domain has the score NaN and drops the sample
    pair like any NaN.  No shift can be given (the scores are centred if the marginals fit), and M <= 1023.

    Per level l and kept sample k, with f_k / c_k the fine / coarse component vectors and a the shift (the same for every
    level, fine and coarse, so the levels telescope):
        Y_k = (f_k - a)(f_k - a)^T - (c_k - a)(c_k - a)^T          (level 0: Y_k = (f_k - a)(f_k - a)^T)
    estimate_mean gives the level sums s_l = sum_k Y_k and sp_l = sum_k Y_k o Y_k, hence mean, var, l_means, l_vars,
    n_samples and n_rm_samples with their usual meaning.  A sample is dropped from the whole matrix if any of its M fine or
    M coarse values is NaN (mask_nan_samples over the [M, n, 2] chunk).  With a = 0 entry (i, j) is exactly
    estimate_mean(q_i * q_j) (the reference's route: one derived quantity per pair).  Each stored chunk is read once by one
    launch of the fp64 matrix-core kernel (mlmc_amd/csrc/xcov.hip) for all M (M + 1) / 2 pairs.

    :param quantity: Quantity with M <= 1024 scalar components (not a moments / covariance node)
    :param shift: None (zeros) or M finite values
    """
    limit, note = engine.ComponentCovAccumulator.MAX_COMPONENTS, ""
    if scores is not None:
        limit, note = limit - 1, " with scores"                  # the row of ones takes one of the accumulator's rows
    M, shift, scores = _component_args("component_covariance", quantity, shift, scores, limit, note)
    side = M if scores is None else M + 1
    return _ComponentCovNode(quantity, shift, qt.ArrayType(shape=(side, side), qtype=qt.ScalarType()), scores=scores)


def _component_args(what, quantity, shift, scores, max_components, limit_note="", limit_first=False):
    """The checks of `shift` / `scores` that component_covariance and bootstrap_component_covariance share; `what` names the caller
    in the messages, `limit_note` ends the one about max_components, which comes before (limit_first) or between the checks of the
    scores, as each caller always had it.  -> M, shift as a float64 array [M] | None, scores as a list | None"""
    if not isinstance(quantity, qmod.Quantity) or isinstance(quantity, (_MomentsNode, _CovarianceNode, _ComponentCovNode)):
        raise TypeError("{}: needs a Quantity whose samples are component values, got {}".format(what, type(quantity).__name__))
    M = int(quantity.size())
    if scores is not None and not (limit_first and M > max_components):
        scores = list(scores)
        if shift is not None:
            raise ValueError("{}: scores and shift exclude each other".format(what))
        if len(scores) != M:
            raise ValueError("{}: {} score distributions for {} components".format(what, len(scores), M))
    if M > max_components:
        raise ValueError("{}: {} components, at most {} are supported{}".format(what, M, max_components, limit_note))
    if scores is not None and (len({d.n_intervals for d in scores}) != 1 or len({d._gauss_degree for d in scores}) != 1):
        raise ValueError("{}: every distribution must use the same quadrature".format(what))
    if shift is not None:
        shift = np.array(shift, dtype=np.float64)
        if shift.shape != (M,):
            raise ValueError("{}: shift of shape {}, expected ({},)".format(what, shift.shape, M))
        if not np.all(np.isfinite(shift)):
            raise ValueError("{}: the shift must be finite".format(what))
    return M, shift, scores


def moment(quantity, moments_fn, i=0):
    """Quantity of the i-th moment function of `quantity` (reference: quantity_estimate.py:83-93)."""
    return qmod.Quantity(quantity_type=quantity.qtype, input_quantities=[quantity],
                         operation=lambda x: moments_fn.eval_single_moment(i, value=x))


def moments(quantity, moments_fn, mom_at_bottom=True):
    """Quantity of all moment functions (reference: quantity_estimate.py:96-119)."""
    if mom_at_bottom:
        qtype = quantity.qtype.replace_scalar(qt.ArrayType(shape=(moments_fn.size,), qtype=qt.ScalarType()))
    else:
        qtype = qt.ArrayType(shape=(moments_fn.size,), qtype=quantity.qtype)
    return _MomentsNode(quantity, moments_fn, mom_at_bottom, qtype)


def covariance(quantity, moments_fn, cov_at_bottom=True):
    """Quantity of the moment outer products (reference: quantity_estimate.py:122-156)."""
    shape = (moments_fn.size, moments_fn.size)
    if cov_at_bottom:
        qtype = quantity.qtype.replace_scalar(qt.ArrayType(shape=shape, qtype=qt.ScalarType()))
    else:
        qtype = qt.ArrayType(shape=shape, qtype=quantity.qtype)
    return _CovarianceNode(quantity, moments_fn, cov_at_bottom, qtype)


class _DeviceChunkCache:
    """HBM-resident copies of the raw sample chunks an estimate has consumed (LRU, bounded).

    An MLMC post-processing session runs several passes over the same samples (moments, covariance, level variances,
    the two passes of construct_density); the first pass uploads each chunk once, later passes -- and later estimates of
    the same quantity -- read it from HBM, where a whole multi-level estimate is one kernel launch.  288 GB of HBM3E
    hold 1.8e10 sample pairs; the default budget is MLMC_HIP_DEVICE_CACHE_GB = 64.
    Keyed by (source quantity, level, chunk id, chunk slice, stamp of the level = samples collected + the storage's
    modification count where it keeps one, _level_stamps): storages are append-only, so a level that has grown misses and
    is uploaded again.  `device_cache_clear()` drops everything."""

    def __init__(self):
        self._items = collections.OrderedDict()
        self._bytes = 0
        self.uploads = 0
        self.hits = 0
        # Every method is a multi-step update of (_items, _bytes): `get` alone is lookup + move_to_end, and a clear() of another
        # thread between the two raises KeyError in the looking thread (the round-2 "hang" of
        # test_concurrent_estimates_through_the_python_api).  Callers hold _estimate_lock as well; the
        # cache does not rely on that.
        self._lock = threading.RLock()

    @staticmethod
    def budget():
        return int(float(os.environ.get("MLMC_HIP_DEVICE_CACHE_GB", "64")) * 2 ** 30)

    @staticmethod
    def _owner_ref(owner):
        """The cache must not keep a storage (and its host arrays) alive: entries hold a WEAK reference to their owner and
        count only while it lives -- a dead owner's id may be recycled, a live one's cannot.  (Objects that cannot be weakly
        referenced are held strongly, as before.)"""
        if owner is None:
            return None
        import weakref
        try:
            return weakref.ref(owner)
        except TypeError:
            return lambda owner=owner: owner

    @staticmethod
    def _alive(item):
        return item[3] is None or item[3]() is not None

    def get(self, key):
        with self._lock:
            item = self._items.get(key)
            if item is not None and not self._alive(item):
                self.drop(key)                                   # its storage is gone: the rows are garbage now
                item = None
            if item is not None:
                self._items.move_to_end(key)
                self.hits += 1
            return item

    def __contains__(self, key):
        with self._lock:
            item = self._items.get(key)
            return item is not None and self._alive(item)

    def put(self, key, fine, coarse, owner=None):
        nbytes = fine.nbytes + (0 if coarse is None else coarse.nbytes)
        if nbytes > self.budget():
            return None
        item = (_upload(fine, count=False), None if coarse is None else _upload(coarse, count=False), nbytes, self._owner_ref(owner))
        with self._lock:
            self._insert(key, item, nbytes)
            self.uploads += 1
        return item

    def put_tensors(self, key, fine, coarse, owner=None):
        """Cache tensors that already live on the device (results of a lowered quantity, stored rows)."""
        nbytes = fine.numel() * 8 + (0 if coarse is None else coarse.numel() * 8)
        item = (fine, coarse, nbytes, self._owner_ref(owner))
        if nbytes > self.budget():
            return item
        with self._lock:
            self._insert(key, item, nbytes)
        return item

    def _insert(self, key, item, nbytes):
        self.drop(key)                                   # a replaced entry gives its bytes back first
        self._inserts = getattr(self, "_inserts", 0) + 1
        if self._inserts % 64 == 0 or self._bytes + nbytes > self.budget():
            self.drop_dead()                             # rows of storages that no longer exist
        while self._bytes + nbytes > self.budget() and self._items:
            _, (_, _, old, _) = self._items.popitem(last=False)
            self._bytes -= old
        self._items[key] = item
        self._bytes += nbytes

    def drop(self, key):
        with self._lock:
            item = self._items.pop(key, None)
            if item is not None:
                self._bytes -= item[2]

    def drop_dead(self):
        with self._lock:
            for key in [k for k, item in self._items.items() if not self._alive(item)]:
                self.drop(key)

    def drop_owner(self, owner):
        with self._lock:
            for key in [k for k, item in self._items.items() if item[3] is not None and item[3]() is owner]:
                self.drop(key)

    def clear(self):
        with self._lock:
            self._items.clear()
            self._bytes = 0


def _lib_device():
    from .. import _lib
    _lib.lib()
    return _lib._bound_device


@functools.lru_cache(maxsize=None)
def _cuda_device(index):
    import torch
    return torch.device("cuda", index)


_device_cache = _DeviceChunkCache()
# One estimate at a time: one GPU stream, one sample cache, one memo of chunk evaluations shared by all quantities.
_estimate_lock = threading.RLock()


_cache_generation = 0


def device_cache_generation():
    """Counts device_cache_clear() calls: results derived from resident samples (Estimate's kept covariance sums) are
    valid for one generation."""
    return _cache_generation


def device_cache_clear():
    """Drop the HBM-resident sample chunks (call after modifying stored samples in place).  Waits for a running estimate of
    another thread: its kernels may still read the resident rows."""
    global _cache_generation
    with _estimate_lock:
        _cache_generation += 1
        _device_cache.clear()
        _block_meta.clear()


def device_cache_drop_owner(storage):
    """Drop the resident chunks that came from one storage (it changed: grew, was refilled)."""
    with _estimate_lock:
        _device_cache.drop_owner(storage)
        _block_meta.drop_owner(storage)


class _LevelStreamer:
    """Streaming feed of a level that the storage delivers in many chunks (SampleStorageHDF reads one
    `collected_values[chunk_slice]` per chunk and reopens the file every time, mlmc/tool/hdf5.py:353-376,
    sample_storage_hdf.py:169-184): the chunks -- [n][2][M] record arrays, the layout of the reference's Memory storage and of
    HDF5 `collected_values` -- are read by several helper threads straight into PINNED staging blocks of
    MLMC_HIP_STREAM_BLOCK_MB (default 32), a block goes to HBM as ONE asynchronous DMA at link speed while the helpers fill
    the next blocks, and the whole level lands in ONE device tensor in the storage's own layout: the quantity tree then runs
    as one k_expr launch per level (strided LOAD: fine / coarse de-interleaving and the row gather on the device), every
    other quantity of the analysis finds the level resident.  Reads (h5py, NumPy copies) and the copies into the staging
    blocks release the GIL, so the helpers really run side by side; per chunk the main thread does nothing.
    MLMC_HIP_STREAM_THREADS (default 4: more helpers contend for the page-fault lock and the GIL and lose) helpers; MLMC_HIP_STREAM_UPLOAD=0 switches the feed off (chunk by chunk, synchronously).

    (Round 2 had a read-ahead thread that handed single chunks to the main thread -- one pageable copy, one k_expr launch and
    ~100 us of Python per 1.6 MB chunk: 16 GB/s -- and an opt-in ring of chunk-sized pinned buffers whose per-chunk
    asynchronous copy + event cost as much host time as the synchronous copy: 0.9 GB/s.  Both are gone.)"""
    N_BUF = 3

    def __init__(self):
        self._pinned = [None] * self.N_BUF
        self._stream = None
        self.blocks = 0            # staging blocks sent (tests)
        self.levels = 0

    @staticmethod
    def enabled():
        return os.environ.get("MLMC_HIP_STREAM_UPLOAD", "1") != "0"

    @staticmethod
    def block_doubles():
        return max(int(float(os.environ.get("MLMC_HIP_STREAM_BLOCK_MB", "32")) * 2 ** 20) // 8, 1)

    @staticmethod
    def n_threads():
        return max(int(os.environ.get("MLMC_HIP_STREAM_THREADS", "4")), 1)

    def _buffer(self, slot, doubles):
        import torch
        buf = self._pinned[slot]
        if buf is None or buf.numel() < doubles:
            buf = self._pinned[slot] = torch.empty(doubles, dtype=torch.float64, pin_memory=True)
        return buf

    def stream(self, leaf, levels, n_rows_read, budget_bytes):
        """levels: [(level id, [chunk specs of the level])].  Generator of (level id, block | None, first chunk | None) in the
        order given: block = (flat device tensor, sample stride, side stride, n, width) once the level has landed; None when
        the level does not qualify (unknown chunk sizes, not record arrays, too large) -- the caller then takes its chunks one
        by one and must not read the first one again (it is handed back).  The levels are ONE pipeline: while the last block of
        a level is on its way (and the caller queues the level's kernels) the helpers already fill the next level's blocks."""
        import torch
        plans = []                      # per qualifying level: dict(level, specs, sizes, sn, sw, m_total, width, raw0, out, blocks...)
        early = []
        for level_id, specs in levels:
            sizes = []
            for cs in specs:
                sl = cs.chunk_slice
                if sl is None or sl.start is None or sl.stop is None or sl.step not in (None, 1):
                    sizes = None
                    break
                sizes.append(sl.stop - sl.start)
            if sizes is None:
                early.append((level_id, None, None))
                continue
            raw0 = leaf.samples(specs[0])
            # (a one-row storage whose chunk already is an [n][2] row counts as a record array with M = 1 here)
            layout = _block_layout(raw0, n_rows_read, True) if raw0.ndim == 3 and raw0.shape[1] == sizes[0] else None
            n_total = sum(sizes)
            if layout is None or n_total * layout[1] * 8 > budget_bytes or max(sizes) * layout[1] > 16 * self.block_doubles():
                early.append((level_id, None, raw0))
                continue
            plans.append(dict(level=level_id, specs=specs, sizes=sizes, sn=layout[1], sw=layout[2], m_total=raw0.shape[0],
                              width=raw0.shape[2], raw0=raw0, n_total=n_total))
        for item in early:
            yield item
        if not plans:
            return
        dev = _cuda_device(_lib_device())
        cap = max([self.block_doubles()] + [max(p["sizes"]) * p["sn"] for p in plans])
        # global lists: tasks (one per chunk, in order) and staging blocks (consecutive chunks of ONE level)
        tasks, blocks = [], []          # task: (plan index, chunk index, block index, offset in block); block: [plan index, length, tasks left, offset in level]
        for pi, p in enumerate(plans):
            p["out"] = torch.empty(p["n_total"] * p["sn"], dtype=torch.float64, device=dev)
            cur_len, pos = 0, 0
            blocks.append([pi, 0, 0, 0])
            for ci, n_c in enumerate(p["sizes"]):
                need = n_c * p["sn"]
                if cur_len and cur_len + need > cap:
                    pos += cur_len
                    blocks.append([pi, 0, 0, pos])
                    cur_len = 0
                tasks.append((pi, ci, len(blocks) - 1, cur_len))
                cur_len += need
                blocks[-1][1] = cur_len
                blocks[-1][2] += 1
            p["last_block"] = len(blocks) - 1
        views = [self._buffer(k, cap).numpy() for k in range(min(self.N_BUF, len(blocks)))]
        # storages that can write a chunk's [n][2][M] records straight into a caller buffer (sample_storage.Memory
        # .sample_records_into; an HDF5 storage: Dataset.read_direct) skip the intermediate array: one host copy, no fresh pages
        into = getattr(getattr(leaf, "_storage", None), "sample_records_into", None)
        if os.environ.get("MLMC_HIP_STREAM_READ_INTO", "1") == "0":
            into = None
        for p in plans:
            p["into"] = into is not None and p["sn"] == 2 * p["m_total"] and (p["width"] == 1 or p["sw"] == p["m_total"])
        cond = threading.Condition()
        state = {"next": 0, "released": 0, "error": None}
        ready = [threading.Event() for _ in blocks]

        def worker():
            while True:
                with cond:
                    if state["error"] is not None or state["next"] >= len(tasks):
                        return
                    pi, ci, b, off = tasks[state["next"]]
                    state["next"] += 1
                    while b >= state["released"] + self.N_BUF and state["error"] is None:   # its slot still holds an older block
                        cond.wait(0.05)
                    if state["error"] is not None:
                        return
                try:
                    p = plans[pi]
                    if p["into"] and ci > 0:                     # (chunk 0 was read as an array to learn the layout)
                        n_c = p["sizes"][ci]
                        into(p["specs"][ci], views[b % self.N_BUF][off:off + n_c * p["sn"]].reshape(n_c, 2, p["m_total"]))
                        with cond:
                            blocks[b][2] -= 1
                            done = blocks[b][2] == 0
                        if done:
                            ready[b].set()
                        continue
                    raw = p["raw0"] if ci == 0 else leaf.samples(p["specs"][ci])
                    lay = _block_layout(raw, n_rows_read, True) if raw.ndim == 3 else None
                    if raw.shape != (p["m_total"], p["sizes"][ci], p["width"]) or lay is None or lay[1:] != (p["sn"], p["sw"]):
                        raise ValueError("chunk {} of level {} does not continue the record layout of the level's first chunk"
                                         .format(p["specs"][ci].chunk_id, p["specs"][ci].level_id))
                    span = (p["sizes"][ci] - 1) * p["sn"] + (p["width"] - 1) * p["sw"] + p["m_total"]
                    flat = np.lib.stride_tricks.as_strided(raw, shape=(span,), strides=(8,))
                    np.copyto(views[b % self.N_BUF][off:off + span], flat)
                except BaseException as e:                       # noqa: BLE001 - handed to the consumer
                    with cond:
                        state["error"] = e
                        cond.notify_all()
                    for ev in ready:
                        ev.set()
                    return
                with cond:
                    blocks[b][2] -= 1
                    done = blocks[b][2] == 0
                if done:
                    ready[b].set()

        threads = [threading.Thread(target=worker, name="mlmc-level-reader", daemon=True)
                   for _ in range(min(self.n_threads(), len(tasks)))]
        for t in threads:
            t.start()
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=dev)
        try:
            for b, (pi, length, _, pos) in enumerate(blocks):
                ready[b].wait()
                if state["error"] is not None:
                    raise state["error"]
                p = plans[pi]
                with torch.cuda.stream(self._stream):
                    p["out"][pos:pos + length].copy_(self._pinned[b % self.N_BUF][:length], non_blocking=True)
                self._stream.synchronize()                       # the helpers fill the other slots meanwhile
                with cond:
                    state["released"] = b + 1
                    cond.notify_all()
                self.blocks += 1
                if b == p["last_block"]:
                    self.levels += 1
                    yield p["level"], (p["out"], p["sn"], p["sw"], p["n_total"], p["width"]), None
        except BaseException:
            with cond:
                if state["error"] is None:
                    state["error"] = RuntimeError("level stream aborted")
                cond.notify_all()
            raise
        finally:
            for t in threads:
                t.join()


_streamer = _LevelStreamer()


def _upload(host_array, count=True):
    """Host array (any shape, float64, C-contiguous) -> device tensor of the same shape, as one synchronous pageable copy (a
    whole level in one chunk goes up at link speed that way; many-chunk levels take the _LevelStreamer)."""
    import torch
    a = np.ascontiguousarray(host_array, dtype=np.float64)
    if count:
        _device_cache.uploads += 1
    dev = _cuda_device(_lib_device())
    t = torch.from_numpy(a).to(dev)
    torch.cuda.current_stream(dev).synchronize()                 # the library reads it on its own stream
    return t


class _ChunkPrefetcher:
    """Read-ahead for the chunks the _LevelStreamer does not take (levels whose chunks are not record arrays -- their rows go
    up one by one --, partly resident levels, chunk specs without slices): a helper thread reads the chunks the estimate is
    going to miss, in order, up to `depth` ahead of the consumer, while the main thread uploads the previous chunk and queues
    its kernels; per chunk the feed costs max(read, upload) instead of their sum.  MLMC_HIP_STREAM_UPLOAD=0 switches it off."""

    def __init__(self, leaf, specs, depth=2):
        import queue
        self._leaf = leaf
        self._specs = list(specs)
        self._queue = queue.Queue(maxsize=depth)
        self._stop = False
        self._thread = threading.Thread(target=self._run, name="mlmc-chunk-reader", daemon=True)
        self._thread.start()

    @staticmethod
    def enabled():
        return os.environ.get("MLMC_HIP_STREAM_UPLOAD", "1") != "0"

    def _run(self):
        try:
            for spec in self._specs:
                if self._stop:
                    return
                self._queue.put((spec, self._leaf.samples(spec), None))
        except BaseException as e:                                # noqa: BLE001 - handed to the consumer
            self._queue.put((None, None, e))

    def get(self, spec):
        """The chunk of `spec`; specs must be asked for in the order they were given."""
        got, raw, err = self._queue.get()
        if err is not None:
            raise err
        assert got is spec or (got.level_id, got.chunk_id) == (spec.level_id, spec.chunk_id)
        return raw

    def close(self):
        self._stop = True
        try:
            while True:
                self._queue.get_nowait()
        except Exception:
            pass


def _split_fine_coarse(chunk, level_id):
    """[M, n, 2|1] -> contiguous fine[M, n], coarse[M, n] | None (level 0 carries no coarse samples)."""
    fine = np.ascontiguousarray(chunk[:, :, 0], dtype=np.float64)
    if level_id == 0 or chunk.shape[-1] == 1:
        return fine, None
    return fine, np.ascontiguousarray(chunk[:, :, 1], dtype=np.float64)


class _AccumulatorPool:
    """Finished LevelAccumulators, reused by the next estimate with the same (moment functions, levels, mode,
    components): creating one allocates device state, scratch and a pinned mirror (~0.3 ms), an estimate over resident
    samples takes about as long."""

    def __init__(self, capacity=8):
        self._items = collections.OrderedDict()
        self._capacity = capacity

    def take(self, fn, n_levels, mode, n_comp, mean_only=False):
        key = (id(fn), n_levels, mode, n_comp, bool(mean_only))
        item = self._items.pop(key, None)
        if item is not None:
            acc = item[0]
            acc.reset()
            return acc
        if mode == engine.LevelAccumulator.COMPONENT_COV:         # (fn is None: pooled by components, levels, mean_only)
            return engine.ComponentCovAccumulator(n_comp, n_levels, mean_only=mean_only)
        return engine.LevelAccumulator(fn, n_levels, mode, n_comp=n_comp, mean_only=mean_only)

    def give(self, fn, n_levels, mode, n_comp, acc, mean_only=False):
        self._items[(id(fn), n_levels, mode, n_comp, bool(mean_only))] = (acc, fn)     # fn kept alive: its id stays unique
        while len(self._items) > self._capacity:
            _, (old, _) = self._items.popitem(last=False)
            old.close()

    def clear(self):
        for acc, _ in self._items.values():
            acc.close()
        self._items.clear()


_acc_pool = _AccumulatorPool()


def _device_tree_enabled():
    return os.environ.get("MLMC_HIP_DEVICE_TREE", "1") != "0"


def _owner_of(plan):
    """The object whose lifetime bounds the resident rows / blocks of a lowered tree: the storage behind the leaf, or the
    leaf itself when it has none.  ONE rule for the upload paths, the residency check of the prefetcher and the cache keys."""
    storage = getattr(plan.leaf, "_storage", None)
    return storage if storage is not None else plan.leaf


def _stored_row_on_device(plan, chunk_spec, chunk_key, stored_row, use_cache, raw=None):
    """One stored row of one chunk as a device tensor in the storage's own layout: interleaved (fine, coarse) pairs
    [n, 2], or [n, 1] at level 0.  Uploaded once per (storage, chunk, row) and shared by every quantity that reads it."""
    import torch
    storage = getattr(plan.leaf, "_storage", None)
    owner = _owner_of(plan)
    key = ("row", id(owner)) + chunk_key + (stored_row,)
    item = _device_cache.get(key) if use_cache else None
    if item is not None:
        return item[0]
    if hasattr(storage, "device_row"):                            # samples that already live in HBM (sim/synth_device.py)
        t = storage.device_row(chunk_spec, stored_row)
    else:
        if raw is None:
            raw = plan.leaf.samples(chunk_spec)                   # [M_stored, n, 2|1]
        t = _upload(raw[stored_row])
    if use_cache:
        _device_cache.put_tensors(key, t, None, owner=owner)
    return t


def _block_layout(raw, n_rows_read, ready_rows_too=False):
    """Can the chunk view raw [M_stored, n, 2|1] go to the device as one flat copy of the storage's [n][sides][M] records?
    -> (span in doubles from the first to the last value, sample stride, side stride) or None (rows are uploaded one by
    one: they already are contiguous [n][2] / [n] rows, the tree reads less than 1/8 of a wide record, or the view is not
    a record array).  Pure layout arithmetic on shape and strides."""
    m_total, n, width = raw.shape
    if n == 0 or raw.dtype != np.float64 or any(st % 8 for st in raw.strides):
        return None
    sm, sn, sw = (st // 8 for st in raw.strides)
    if m_total == 1:
        sm = 1                                                   # the stride of a length-1 axis carries no meaning
    if width == 1:
        sw = 0
    rows_are_ready = (sn == width and (width == 1 or sw == 1))   # raw[m] already is an [n][2] / [n] row
    if (rows_are_ready and not ready_rows_too) or (m_total > 1 and n_rows_read * 8 < m_total):
        return None
    if sm != 1 or sn < m_total * width or (width == 2 and sw < m_total):
        return None                                              # not an [n][sides][M] record array
    span = (n - 1) * sn + (width - 1) * sw + m_total              # doubles between the first and the last value
    if span > 3 * raw.size:
        return None
    return span, sn, sw


class _BlockMeta:
    """(block key [, rows the tree reads]) -> (sample stride, side stride, n, width) of a resident block, or None when the
    chunk is uploaded row by row: a later estimate decides without reading the chunk from the storage again.  The keys
    carry id(owner); every entry also holds a weak reference to that owner and counts only while it is the same live
    object -- a new storage that happens to get the id of a freed one inherits nothing."""
    _MISSING = object()

    def __init__(self):
        self._d = {}

    @staticmethod
    def _ref(owner):
        import weakref
        try:
            return weakref.ref(owner)
        except TypeError:                     # not weak-referenceable: keep it alive, its id then stays unique
            return lambda owner=owner: owner

    def get(self, key, owner, default=_MISSING):
        entry = self._d.get(key)
        if entry is None or entry[0]() is not owner:
            if entry is not None:
                del self._d[key]
            return default
        return entry[1]

    def has(self, key, owner):
        return self.get(key, owner) is not self._MISSING

    def put(self, key, owner, value):
        if len(self._d) > 65536:
            self._d.clear()
        self._d[key] = (self._ref(owner), value)

    def drop_owner(self, owner):
        oid = id(owner)
        for key in [k for k in self._d if k[1] == oid]:
            del self._d[key]

    def clear(self):
        self._d.clear()

    def __len__(self):
        return len(self._d)


_block_meta = _BlockMeta()


def _stored_block_on_device(plan, chunk_spec, chunk_key, use_cache, raw=None):
    """The whole stored chunk as ONE device buffer in the storage's own [n][2][M] layout (reference Memory storage and
    HDF5 `collected_values`, sample_storage.py:169-184), when the host view allows it: -> (flat device tensor,
    sample stride, side stride, n, width) or None.  One contiguous PCIe copy replaces one strided host gather per
    stored row (a row of an [n][2][M] array touches a separate cache line per value once M >= 8); k_expr de-interleaves
    while loading (strided LOAD).  Taken when the tree reads at least 1/8 of the stored rows -- and for M = 1 at level 0,
    where the storage keeps an unused coarse column ([n][2], the fine values at stride 2): copying 2x the bytes at link
    speed beats a strided host gather of half of them (2.8 ms vs 8 ms + 1.4 ms for 10^7 samples)."""
    import torch
    storage = getattr(plan.leaf, "_storage", None)
    if hasattr(storage, "device_row") or os.environ.get("MLMC_HIP_BLOCK_UPLOAD", "1") == "0":
        return None
    owner = _owner_of(plan)
    key = ("block", id(owner)) + chunk_key
    item = _device_cache.get(key) if use_cache else None
    if use_cache and (_block_meta.has(key + ("any",), owner) or _block_meta.has(key + (len(plan.in_rows),), owner)):
        return None                                               # known: the chunk goes up row by row (for any / this many rows)
    if item is not None and _block_meta.has(key, owner):
        return (item[0],) + _block_meta.get(key, owner)           # a resident block serves every tree
    if raw is None:
        raw = plan.leaf.samples(chunk_spec)                       # [M_stored, n, 2|1] view of the storage / fresh read
    layout = _block_layout(raw, len(plan.in_rows))
    if layout is None or layout[0] * 8 > _DeviceChunkCache.budget() // 4:
        if use_cache:                                             # not a record array at all, or too few of its rows are read
            intrinsic = layout is not None or _block_layout(raw, raw.shape[0]) is None
            _block_meta.put(key + (("any",) if intrinsic else (len(plan.in_rows),)), owner, None)
        return None
    span, sn, sw = layout
    m_total, n, width = raw.shape
    if item is None:
        flat = np.lib.stride_tricks.as_strided(raw, shape=(span,), strides=(8,))
        t = _upload(flat)
        if use_cache:
            _device_cache.put_tensors(key, t, None, owner=owner)
            _block_meta.put(key, owner, (sn, sw, n, width))
    else:
        t = item[0]
    return t, sn, sw, n, width


def _level_blocks_on_device(plan, owner, levels, n_collected, use_cache, first_raw):
    """The stored samples of whole levels as one device tensor each, in the storage's [n][2][M] layout, for levels the storage
    hands out in several chunks: resident from an earlier estimate of any quantity over the same storage, or streamed now
    (_LevelStreamer, all levels as one pipeline).  levels: [(level id, [chunk specs])].  Generator of
    (level id, (flat tensor, sample stride, side stride, n, width)); levels that do not qualify are skipped (they are taken
    chunk by chunk; a first chunk that was read on the way is left in `first_raw` for that path)."""
    to_stream = []
    for level_id, level_specs in levels:
        stamp = None if n_collected is None else n_collected[level_id]
        key = ("lvlblock", id(owner), level_id, stamp)
        if use_cache:
            item = _device_cache.get(key)
            if item is not None and _block_meta.has(key, owner):
                yield level_id, (item[0],) + _block_meta.get(key, owner)
                continue
            if _block_meta.has(key + ("no", len(plan.in_rows)), owner):
                continue                                          # known: this level does not stream for a tree of that many rows
        if len(level_specs) < 2 or not _LevelStreamer.enabled() or os.environ.get("MLMC_HIP_BLOCK_UPLOAD", "1") == "0":
            continue
        if use_cache:                                             # a level that is partly resident keeps its chunk-wise path
            partly = False
            for cs in level_specs:
                ck = _chunk_key(None, cs, n_collected)[1:]
                if (("block", id(owner)) + ck) in _device_cache or any((("row", id(owner)) + ck + (r,)) in _device_cache for r in plan.in_rows):
                    partly = True
                    break
            if partly:
                continue
        to_stream.append((level_id, level_specs))
    if not to_stream:
        return
    first_spec = {level_id: specs[0] for level_id, specs in to_stream}
    for level_id, got, raw0 in _streamer.stream(plan.leaf, to_stream, len(plan.in_rows), _DeviceChunkCache.budget() // 4):
        stamp = None if n_collected is None else n_collected[level_id]
        key = ("lvlblock", id(owner), level_id, stamp)
        if got is None:
            if raw0 is not None:
                first_raw[id(first_spec[level_id])] = raw0
            if use_cache:
                _block_meta.put(key + ("no", len(plan.in_rows)), owner, None)
            continue
        _device_cache.uploads += 1
        if use_cache:
            _device_cache.put_tensors(key, got[0], None, owner=owner)
            _block_meta.put(key, owner, got[1:])
        yield level_id, got


def _evaluate_on_device(plan, chunk_spec, chunk_key, use_cache, raw=None):
    """Result rows of a lowered quantity for one chunk: fine [M, n'], coarse [M, n'] | None (torch CUDA tensors).
    raw: the chunk as the storage returned it, when a prefetcher has read it already."""
    blk = _stored_block_on_device(plan, chunk_spec, chunk_key, use_cache, raw)
    if blk is not None:
        t, sn, sw, n, width = blk
        # without the cache nothing keeps the uploaded block alive past this call: wait for the kernel that reads it
        fine, coarse, _ = plan.evaluate([t[r:] for r in plan.in_rows], has_coarse=(width == 2), n=n, sample_stride=sn,
                                        side_stride=max(sw, 1), sync=not use_cache)
        return fine, coarse
    storage = getattr(plan.leaf, "_storage", None)
    if raw is None and not hasattr(storage, "device_row"):
        owner = _owner_of(plan)
        if not use_cache or any(("row", id(owner)) + chunk_key + (r,) not in _device_cache for r in plan.in_rows):
            raw = plan.leaf.samples(chunk_spec)                  # ONE read of the chunk for all its rows
    rows = [_stored_row_on_device(plan, chunk_spec, chunk_key, r, use_cache, raw) for r in plan.in_rows]
    n, width = rows[0].shape
    if n == 0:
        return None
    if width == 1 and plan.is_row_copy:
        return rows[0].view(1, n), None         # a level-0 row already is the contiguous fine array: no kernel, no copy
    fine, coarse, _ = plan.evaluate(rows, has_coarse=(width == 2), n=n, sync=not use_cache)
    return fine, coarse


def _cache_ident(source, plan):
    """Identity of a quantity's rows in the device cache: (storage, lowered program) for lowered trees -- equivalent
    trees (rebuilt quantity objects, a second make_root_quantity over the same storage) share entries -- else the
    quantity object itself."""
    if plan is not None:
        return (id(_owner_of(plan)), plan.signature)
    return id(source)


def _level_stamps(storage_q):
    """Per level (samples collected, storage version): what the resident rows of a level are valid for.  Storages of the
    reference are append-only, so the count alone identifies a level's contents; mlmc_amd's own Memory storage also counts
    its modifications per level (`_level_versions`), which covers a level that was rebuilt with the same number of samples.  Arrays of a
    foreign storage edited in place are invisible to both: call device_cache_clear() after such an edit."""
    versions = getattr(getattr(storage_q, "_storage", None), "_level_versions", None) or {}
    return tuple((int(c), versions.get(level)) for level, c in enumerate(storage_q.n_collected()))


def _chunk_key(ident, chunk_spec, n_collected):
    sl = chunk_spec.chunk_slice
    return (ident, chunk_spec.level_id, chunk_spec.chunk_id, None if sl is None else (sl.start, sl.stop),
            None if n_collected is None else n_collected[int(chunk_spec.level_id)])


def _merge_level(pairs):
    """The resident chunks of one level as one tensor pair (one device copy), or None when they are not all resident /
    not all of one kind / too large to hold twice for a moment."""
    import torch
    pairs = [p for p in pairs if p is not None and p[0].shape[-1] > 0]
    if len(pairs) < 2 or not all(isinstance(p[0], torch.Tensor) for p in pairs):
        return None
    if len({p[1] is None for p in pairs}) != 1:
        return None
    nbytes = sum(p[0].numel() * 8 * (1 if p[1] is None else 2) for p in pairs)
    if 2 * nbytes > _DeviceChunkCache.budget():
        return None
    from .. import _lib
    _lib.check(_lib.lib().mlmc_synchronize())                     # the chunks may still be being written by k_expr
    fine = torch.cat([p[0] for p in pairs], dim=1).contiguous()
    coarse = None if pairs[0][1] is None else torch.cat([p[1] for p in pairs], dim=1).contiguous()
    torch.cuda.current_stream(fine.device).synchronize()          # the library reads them on its own stream
    return fine, coarse


def _chunk_for_device(source, plan, chunk_spec, n_collected, use_cache, raw=None):
    """Sample rows of `source` for one storage chunk, ready for the accumulators: (fine [M, n], coarse [M, n] | None) as
    torch CUDA tensors (resident: served from / added to the HBM cache) or, when the chunk does not fit the cache budget
    and the tree is evaluated on the host, as NumPy arrays that go through the staging buffer of the C ABI."""
    owner = _owner_of(plan) if plan is not None else source
    ident = _cache_ident(source, plan)
    key = _chunk_key(ident, chunk_spec, n_collected)
    item = _device_cache.get(key) if use_cache else None
    if item is not None:
        return item[0], item[1]
    if plan is not None:
        got = _evaluate_on_device(plan, chunk_spec, key[1:], use_cache, raw)
        if got is None:
            import torch
            return torch.empty((plan.n_out, 0), dtype=torch.float64), None
        if use_cache:
            _device_cache.put_tensors(key, got[0], got[1], owner=owner)
        return got
    raw = source.samples(chunk_spec)                             # [M, n, 2|1], host evaluation of the tree
    if raw.shape[1] == 0:
        return np.empty((raw.shape[0], 0)), None
    fine, coarse = _split_fine_coarse(raw, chunk_spec.level_id)
    item = _device_cache.put(key, fine, coarse, owner=source) if use_cache else None
    if item is None:
        return fine, coarse                                      # not cached: staged through the C ABI
    return item[0], item[1]


# What a walk over the stored chunks of a quantity settles before the first chunk: the storage that hands out the chunk specs, the
# lowered tree of the rows that are read (None: evaluated on the host), the stamps of the levels (None: the storage cannot tell),
# whether chunks are served from / added to the device cache, and for its keys the identity of the rows and the object whose
# lifetime bounds them; the torch device of the library.
_Walk = collections.namedtuple("_Walk", "storage_q n_levels plan n_collected use_cache ident owner dev")


def _walk_setup(quantity, source=None):
    """The _Walk of estimate_mean, the per-component entries and the bootstraps.  The memo of host evaluations is cleared; the rows
    of `source` -- the quantity whose chunks are read: `quantity` itself, or for an estimate the input of its moments / covariance
    node -- are cached when there is a budget, the storage stamps its levels and the rows are not a fresh random draw per
    evaluation (`_volatile`)."""
    source = quantity if source is None else source
    cache_clear()
    storage_q = quantity.get_quantity_storage()
    n_levels = int(max(storage_q.level_ids())) + 1
    # a tree of per-sample nodes runs as one device program over the stored rows (quantity/lowering.py)
    plan = lowering.plan_for(source) if _device_tree_enabled() else None
    try:
        n_collected = _level_stamps(storage_q)
    except Exception:
        n_collected = None
    use_cache = _DeviceChunkCache.budget() > 0 and n_collected is not None and not getattr(source, "_volatile", False)
    return _Walk(storage_q, n_levels, plan, n_collected, use_cache, _cache_ident(source, plan),
                 _owner_of(plan) if plan is not None else source, _cuda_device(_lib_device()))


def _device_rows(x, M, dev):
    """x: [M, n] values, a host array or a tensor -> (contiguous float64 tensor [M, n] on `dev`, whether that took a copy).  A copy
    runs on torch's stream and the library reads on its own: the caller decides when to wait."""
    import torch
    if isinstance(x, torch.Tensor):
        if x.dtype == torch.float64 and x.device == dev and x.dim() == 2 and x.shape[0] == M and x.is_contiguous():
            return x, False                                      # (resident rows: the usual case)
        t = x
    else:
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    rows = t.to(device=dev, dtype=torch.float64).reshape(M, t.shape[-1]).contiguous()
    return rows, rows.data_ptr() != t.data_ptr()


def fine_samples_for_device(quantity, chunk_spec):
    """Fine values of one chunk of `quantity` where the device wants them: a torch CUDA tensor when the tree is lowered
    (stored rows resident or generated in HBM, nothing crosses PCIe), else the host array of the host-evaluated tree.
    Used by Estimate.estimate_domain (percentiles of the fine samples)."""
    with _estimate_lock:
        return _fine_samples_for_device(quantity, chunk_spec)


def _fine_samples_for_device(quantity, chunk_spec):
    plan = lowering.plan_for(quantity) if _device_tree_enabled() else None
    if plan is None:
        return np.squeeze(quantity.samples(chunk_spec)[..., 0])
    storage_q = quantity.get_quantity_storage()
    try:
        n_collected = _level_stamps(storage_q)
    except Exception:
        n_collected = None
    use_cache = _DeviceChunkCache.budget() > 0 and n_collected is not None
    fine, _ = _chunk_for_device(quantity, plan, chunk_spec, n_collected, use_cache)
    return fine


def _subsample_on_device(pair, params):
    """Quantity.pick_samples (reference quantity.py:308-325) on the device: the chunk's share of the k-of-n sub-sample is
    drawn on the host (hypergeometric count, as in the reference), the `size` columns -- uniform with replacement,
    RNG.choice(chunk, size, axis=1) -- are gathered by mlmc_subsample_gather with a counter-based generator."""
    import torch
    from .. import _lib
    fine, coarse = pair
    n = fine.shape[-1]
    # scipy.stats.hypergeom(M = n_total, n = k, N = chunk).rvs() of the reference, drawn with the NumPy generator directly
    # (building a frozen scipy distribution costs ~0.3 ms per chunk, more than the estimate itself)
    size = int(qmod.RNG.hypergeometric(params._orig_k, params._orig_n - params._orig_k, min(n, params._orig_n)))
    seed = int(qmod.RNG.integers(0, 2 ** 63 - 1))
    if not isinstance(fine, torch.Tensor):                       # host chunk (over the cache budget): upload for the gather
        dev = _cuda_device(_lib_device())
        fine = _device_rows(fine, fine.shape[0], dev)[0]
        coarse = None if coarse is None else _device_rows(coarse, coarse.shape[0], dev)[0]
        torch.cuda.current_stream(dev).synchronize()
    m = fine.shape[0]
    out_f = torch.empty((m, size), dtype=torch.float64, device=fine.device)
    out_c = None if coarse is None else torch.empty((m, size), dtype=torch.float64, device=fine.device)
    if size > 0:
        _lib.check(_lib.lib().mlmc_subsample_gather(fine.data_ptr(), None if coarse is None else coarse.data_ptr(), m, n, size,
                                                    seed, out_f.data_ptr(), None if out_c is None else out_c.data_ptr()))
    return out_f, out_c


def _linearized_basis(fn):
    """The larger member of fn's family whose level SUMS give the level sums of fn's moment covariance (linearize.py):
    Legendre / monomial / Fourier moments, `estimate_mean(covariance(q, fn), variance=False)`.  None: the covariance mean
    stays on the matrix cores (splines, transformed moments, sizes the family does not reach; MLMC_HIP_LINEARIZE=0)."""
    if os.environ.get("MLMC_HIP_LINEARIZE", "1") == "0":
        return None
    k_ext = linearize.extended_size(fn)
    if k_ext is None or k_ext > 512:
        return None
    ext = fn.__dict__.get("_lin_ext")
    if ext is None or ext.size != k_ext:
        ext = fn.change_size(k_ext)
        fn.__dict__["_lin_ext"] = ext          # one device handle and one pooled accumulator per moments object
    return ext


def _sums_from_linearized_memo(fn, key, owner):
    """Level sums of TransformedMoments(base, T) from the kept sums of a linearised covariance-mean estimate of `base` over the
    same samples (same quantity rows, same level stamps, same cache generation): the transformed moments are linear in the
    base moments, sum_n (T d_n) = T sum_n d_n, and the keep / drop decision is the base transform's.  This is the second
    pass of Estimate.construct_density (estimator.py:304-331) without a second pass.  -> (n, n_rm, sums [L, n_comp * Rt]) | None"""
    from ..moments import TransformedMoments
    if not isinstance(fn, TransformedMoments) or key is None:
        return None
    memo = fn._base.__dict__.get("_lin_memo")
    if memo is None or memo["key"] != key or fn._base_matrix.shape[1] != memo["R"] or memo["owner"]() is not owner:
        return None                       # (the key carries id(owner): the weak reference rules out a recycled id)
    L, n_comp, K, R = memo["sums"].shape[0], memo["n_comp"], memo["K"], memo["R"]
    base = memo["sums"].reshape(L * n_comp, K)[:, :R]
    return memo["n"].copy(), memo["n_rm"].copy(), (base @ fn._base_matrix.T).reshape(L, -1), n_comp


def linearized_bases(moments_fns):
    """The extended members (_linearized_basis) of M moments objects when ONE pass of mlmc_accum_estimate_multi can serve
    them all -- every one has a linearisation, of the same family and size -- else None (the scalar chain per component)."""
    exts = [_linearized_basis(fn) for fn in moments_fns]
    if not exts or any(e is None for e in exts):
        return None
    if len({type(e) for e in exts}) != 1 or len({e.size for e in exts}) != 1:
        return None
    return exts


def multi_component_sums(quantity, ext_fns):
    """Level sums of the moments ext_fns[m] of row m of `quantity`'s chunks, every component masked on its own, in ONE
    device pass per stored chunk for all components (mlmc_amd/csrc/moments_multi.hip).
    -> n, n_rm [L, M] int64, sums [L, M, K] (K = size of the ext_fns, all equal)"""
    with _estimate_lock:
        return _multi_component_sums(quantity, ext_fns)


def _multi_component_sums(quantity, ext_fns):
    M, K = len(ext_fns), int(ext_fns[0].size)
    return _component_entry(quantity, M, "multi_component_sums", "mlmc_accum_estimate_multi", (M, _basis_handles(ext_fns), K), [(K,)])


def _basis_handles(fns):
    import ctypes as C
    return C.cast((C.c_void_p * len(fns))(*[fn._basis_handle().value for fn in fns]), C.c_void_p)


def _component_chunks(quantity, M, what):
    """The stored chunks of `quantity` as [M, n] float64 device tensors for the per-component entries (mlmc_accum_estimate_multi,
    _var, mlmc_level_diagnostics: _component_entry).
    -> (n_levels, tensors to keep alive until the call returns, (n_chunks, levels, fine, coarse, n_samples) arguments)"""
    import ctypes as C
    import torch
    from .. import _lib
    if quantity.size() != M:
        raise ValueError("{}: {} moments objects for {} components".format(what, M, quantity.size()))
    walk = _walk_setup(quantity)
    levels, fines, coarses, ns, keep = [], [], [], [], []
    for chunk_spec in walk.storage_q.chunks():
        fine, coarse = _chunk_for_device(quantity, walk.plan, chunk_spec, walk.n_collected, walk.use_cache)
        if fine.shape[-1] == 0:
            continue
        fine = _device_rows(fine, M, walk.dev)[0]
        if coarse is not None:
            coarse = _device_rows(coarse, M, walk.dev)[0]
        keep.append((fine, coarse))
        levels.append(int(chunk_spec.level_id))
        fines.append(fine.data_ptr())
        coarses.append(None if coarse is None else coarse.data_ptr())
        ns.append(fine.shape[-1])
    torch.cuda.current_stream(walk.dev).synchronize()
    nc = len(ns)
    lv = np.array(levels, dtype=np.int32)
    nn = np.array(ns, dtype=np.int64)
    fp = (C.c_void_p * max(nc, 1))(*fines)
    cp = (C.c_void_p * max(nc, 1))(*coarses)
    keep.append((lv, nn, fp, cp))
    return walk.n_levels, keep, (nc, _lib.ptr(lv), C.cast(fp, C.c_void_p), C.cast(cp, C.c_void_p), _lib.ptr(nn))


def _component_entry(quantity, M, what, entry, lead, shapes):
    """One call of the per-component C entry `entry` over the stored chunks of `quantity`: entry(*lead, n_levels, the chunk
    arguments, n, n_rm, one float64 output [L, M, *shape] per shape).  -> n, n_rm [L, M] int64, then the float outputs"""
    from .. import _lib
    n_levels, keep, args = _component_chunks(quantity, M, what)
    n = np.zeros((n_levels, M), dtype=np.int64)
    n_rm = np.zeros((n_levels, M), dtype=np.int64)
    outs = [np.zeros((n_levels, M) + shape) for shape in shapes]
    _lib.check(getattr(_lib.lib(), entry)(*lead, n_levels, *args, _lib.ptr(n), _lib.ptr(n_rm), *[_lib.ptr(o) for o in outs]))
    del keep
    return (n, n_rm, *outs)


COMPONENT_FAMILIES = ("Legendre", "Monomial", "Fourier")     # moments of the device route of the per-component estimates


def component_device_route(moments_fns):
    """True when ONE pass of mlmc_accum_estimate_multi_var serves the moments objects of all components: plain Legendre,
    monomial or Fourier moments (own domains, log, safe_eval), all of one family and one size."""
    names = {type(fn).__name__ for fn in moments_fns}
    return len(names) == 1 and names <= set(COMPONENT_FAMILIES) and len({int(fn.size) for fn in moments_fns}) == 1 \
        and int(moments_fns[0].size) <= 512


def component_level_sums(quantity, moments_fns):
    """Level sums of the moments moments_fns[m] of component m (row m of `quantity`'s chunks, masked and clipped on its own) and of
    their squares, ONE device pass per stored chunk for all components (mlmc_accum_estimate_multi_var).
    -> n, n_rm [L, M] int64, s, sp [L, M, R] float64"""
    with _estimate_lock:
        return _component_level_sums(quantity, moments_fns)


def _component_level_sums(quantity, moments_fns):
    M, R = len(moments_fns), int(moments_fns[0].size)
    return _component_entry(quantity, M, "component_level_sums", "mlmc_accum_estimate_multi_var",
                            (M, _basis_handles(moments_fns), R), [(R,), (R,)])


def level_diagnostics(quantity):
    """Central sums of the MLMC convergence diagnostics of every scalar component of `quantity` (any qtype; no moments function):
    per level and component the mean and the central sums of order 2..4 of the level differences, mean and second central sum of
    the fine and of the coarse values and their co-moment (diagnostics.STAT_NAMES), each component NaN-masked on its own
    (mask_nan_samples applied to the one component), two device passes per stored chunk for all components
    (mlmc_level_diagnostics, mlmc_amd/csrc/level_diag.hip).
    -> n, n_rm [L, M] int64, stats [L, M, 9] float64 (for diagnostics.from_central_sums)"""
    with _estimate_lock:
        return _level_diagnostics(quantity)


def _level_diagnostics(quantity):
    from .. import diagnostics
    M = int(quantity.size())
    return _component_entry(quantity, M, "level_diagnostics", "mlmc_level_diagnostics", (M,), [(diagnostics.N_STAT,)])


def component_statistics(n, s, sp):
    """Per-level and total statistics of per-component level sums (n [L, M], s / sp [L, M, R]), as estimate_mean gives them for
    each component alone: engine.level_stats per (level, component), mean = sum_l l_means, var = sum_l l_vars / n_l
    (QuantityMean).  A component without a kept sample raises.  -> l_means, l_vars [L, M, R], mean, var [M, R]"""
    L, M, R = s.shape
    if np.any(np.sum(n, axis=0) == 0):
        raise Exception("All samples were masked")
    l_means, l_vars = engine.level_stats(n.reshape(L * M), s.reshape(L * M, R), sp.reshape(L * M, R))
    l_means, l_vars = l_means.reshape(L, M, R), l_vars.reshape(L, M, R)
    mean = np.sum(l_means, axis=0)
    with np.errstate(all="ignore"):
        var = np.sum(l_vars / n[:, :, None], axis=0)
    return l_means, l_vars, mean, var


def component_estimates(components, moments_fns, cov=False, variance=True):
    """estimate_mean(moments|covariance(components[m], fn_m), variance) of several scalar quantities, component m with
    moments_fns[m], each masked on its own: the per-component loop of the scalar chain.  -> list of QuantityMean"""
    node = covariance if cov else moments
    return [estimate_mean(node(q, fn), variance=variance) for q, fn in zip(components, moments_fns)]


def component_means(components, moments_fns, cov=False):
    """Means of the moments (cov=False: [R] each) or of the moment covariance (True: [R, R]) of several scalar
    quantities, component m with moments_fns[m] -- entry m is estimate_mean(moments|covariance(components[m], fn_m),
    variance=False).mean, each component masked on its own (Estimate.construct_densities)."""
    return [r.mean.reshape((fn.size, fn.size)) if cov else r.mean.reshape(fn.size)
            for r, fn in zip(component_estimates(components, moments_fns, cov=cov, variance=False), moments_fns)]


def estimate_mean(quantity, group=None, variance=True):
    """MLMC mean estimator (reference: quantity_estimate.py:22-80).  Thread-safe: estimates of several host threads are
    serialised (one GPU stream, one sample cache, the memo of chunk evaluations shared by all quantities).

    :param quantity: Quantity
    :param group: optional torch.distributed process group; when a group (or the default group) with more than one
                  rank is initialised every rank passes ITS shard of the samples and the level sums are all-reduced.
    :param variance: False when only `.mean` / `.l_means` will be read (Estimate.construct_density): device passes that
                  exist for the variances alone are skipped and the corresponding variances come back as NaN.
    :return: QuantityMean
    """
    with _estimate_lock:
        return _estimate_mean(quantity, group, variance)


_Target = collections.namedtuple("_Target", "source fn mode rows_per_comp rows_out lin_fn scores shift subsample_params")


def _estimate_target(quantity, variance):
    """What an estimate estimates, from the node at its root: the quantity whose sample rows are read, the moments object (or None),
    accumulator mode and rows per component of the device pass, the rows per component the caller sees, the caller's moments object
    when `fn` is its linearisation, the marginals and the shift of a component covariance, the per-level parameters of
    Quantity.subsample.  No device work; _linearized_basis keeps its extended basis with the moments object."""
    scores = shift = None
    if isinstance(quantity, (_MomentsNode, _CovarianceNode)):
        source = quantity._input_quantities[0]
        fn = quantity._moments_fn
        mode = engine.LevelAccumulator.MOMENTS if isinstance(quantity, _MomentsNode) else engine.LevelAccumulator.COV
        rows_per_comp = fn.size if mode == engine.LevelAccumulator.MOMENTS else fn.size * fn.size
    elif isinstance(quantity, _ComponentCovNode):
        # the raw component values go to the component-covariance accumulator: M x M rows, i.e. M "rows per component"
        source, fn, mode = quantity._input_quantities[0], None, engine.LevelAccumulator.COMPONENT_COV
        scores, shift = quantity._scores, quantity._shift
        rows_per_comp = int(source.size()) + (1 if scores is not None else 0)                # scores: plus the row of ones
    else:
        source, fn, mode, rows_per_comp = quantity, None, engine.LevelAccumulator.MOMENTS, 1
    rows_out = rows_per_comp                                      # rows per component the caller sees
    # Mean of the moment covariance without its variance (Estimate.construct_density): for Legendre / monomial / Fourier
    # moments the R x R level sums are a fixed linear map of the level sums of ~2 R moments of the same family
    # (linearize.py) -- one pass of the moments kernel instead of the matrix-core pass.
    lin_fn = None
    if mode == engine.LevelAccumulator.COV and not variance:
        ext = _linearized_basis(fn)
        if ext is not None:
            lin_fn, fn, mode, rows_per_comp = fn, ext, engine.LevelAccumulator.MOMENTS, ext.size

    # bootstrap sub-sample of a quantity (Quantity.subsample): the chunks of the underlying quantity stay resident in HBM,
    # every estimate draws its random columns on the device (mlmc_subsample_gather)
    subsample_params = None
    sym = source.__dict__.get("_sym")
    if sym is not None and sym[0] == "subsample" and _device_tree_enabled():
        subsample_params = sym[1]
        source = source._input_quantities[0]
    return _Target(source, fn, mode, rows_per_comp, rows_out, lin_fn, scores, shift, subsample_params)


class _ScoreRows:
    """The normal scores of [M, n] device rows under M marginals (simple_distribution._scores_into); the problem arguments are
    built with the first rows.  `what` names the caller in their error messages."""

    def __init__(self, scores, what):
        self._scores, self._what = scores, what
        self._head = self._keep = self._buf = self._width = self._nb = self._ubuf = None

    def _into(self, fine, coarse, n, ld_in, z_fine, z_coarse, u_fine=None, u_coarse=None):
        from ..tool import simple_distribution
        if self._head is None:
            self._head, self._keep = simple_distribution._scores_problem_args(self._scores, self._what)
        simple_distribution._scores_into(self._head, fine, coarse, n, ld_in, z_fine, z_coarse, n, u_fine, u_coarse)

    def uniforms(self, fine, coarse, dev):
        """Generator of (u_fine, u_coarse | None) [M, nc]: the uniforms u = Fhat_m(x) of a pair (the bits of mlmc_density_cdf_batch;
        NaN for NaN and outside the open domain), block by block of score_block_columns(M) columns in one workspace that every block
        reuses -- a block must be consumed before the next one is asked for.  A host chunk is uploaded first, once.  The uniforms
        stay on the device."""
        import torch
        M = len(self._scores)
        if self._ubuf is None:
            self._nb = score_block_columns(M)
            self._ubuf = torch.empty((4, M * self._nb), dtype=torch.float64, device=dev)     # z and u, fine and coarse
        nb = self._nb
        fine = _device_rows(fine, M, dev)[0]
        coarse = None if coarse is None else _device_rows(coarse, M, dev)[0]
        n = int(fine.shape[-1])
        torch.cuda.current_stream(dev).synchronize()                # the library reads and writes on its own stream
        for c0 in range(0, n, nb):
            nc = min(nb, n - c0)
            z_f, z_c, u_f, u_c = [self._ubuf[k, :M * nc].view(M, nc) for k in range(4)]
            if coarse is None:
                self._into(fine[:, c0:], None, nc, n, z_f, None, u_f, None)
                yield u_f, None
            else:
                self._into(fine[:, c0:], coarse[:, c0:], nc, n, z_f, z_c, u_f, u_c)
                yield u_f, u_c

    def chunk(self, fine, coarse, n):
        """The scores of a whole chunk in a workspace of its own (16 M n bytes), which the caller releases.  -> fine, coarse | None"""
        import torch
        ws = torch.empty((2, len(self._scores), n), dtype=torch.float64, device=fine.device)
        torch.cuda.current_stream(fine.device).synchronize()     # the library reads and writes on its own stream
        self._into(fine, coarse, n, n, ws[0], None if coarse is None else ws[1])
        return ws[0], (None if coarse is None else ws[1])

    def blocks(self, fine, coarse, dev):
        """Generator of (fine, coarse | None) [M + 1, nc]: the scores of a pair plus a row of ones, block by block of a fixed number
        of columns (score_block_columns), in one workspace per side that every block reuses -- each block must be pushed before the
        next one is asked for (the library's stream orders a block's push before the next block's scores).  The row of ones sits
        behind the M score rows of a block, so it is rewritten when the width changes.  A host chunk is uploaded first, once."""
        import torch
        from .. import _lib
        M = len(self._scores)
        if self._buf is None:
            self._nb = score_block_columns(M)
            self._buf = torch.empty((2, (M + 1) * self._nb), dtype=torch.float64, device=dev)
        nb = self._nb
        fine = _device_rows(fine, M, dev)[0]
        coarse = None if coarse is None else _device_rows(coarse, M, dev)[0]
        n = int(fine.shape[-1])
        for c0 in range(0, n, nb):
            nc = min(nb, n - c0)
            z = [self._buf[side, :(M + 1) * nc].view(M + 1, nc) for side in range(2)]
            if self._width != nc:
                _lib.check(_lib.lib().mlmc_synchronize())           # earlier pushes have read the workspace
                z[0][M].fill_(1.0)
                z[1][M].fill_(1.0)
                self._width = nc
            torch.cuda.current_stream(dev).synchronize()            # the library reads and writes on its own stream
            self._into(fine[:, c0:], None if coarse is None else coarse[:, c0:], nc, n, z[0], None if coarse is None else z[1])
            yield z[0], (None if coarse is None else z[1])


class _LevelSink:
    """Where the (level, pair) stream of an estimate ends: a pooled accumulator, taken with the first pair.  Resident pairs are
    gathered and handed over in ONE call of the C ABI at the end (mlmc_accum_estimate: reset + pushes + finalize); as soon as a host
    chunk shows up -- it is staged through a reused device buffer and has to be pushed at once -- or the pairs become normal scores,
    everything goes through push() in arrival order."""

    def __init__(self, target, walk, vec_size, variance):
        self._target, self._n_levels, self._dev, self._vec_size = target, walk.n_levels, walk.dev, vec_size
        self._mean_only = not variance
        self._scores = None if target.scores is None else _ScoreRows(target.scores, "component_covariance")
        self._acc = self.n_comp = None
        self._gathered = []
        self._pushed_directly = False

    def push(self, level_id, pair):
        """pair: (fine [M, n], coarse [M, n] | None), device tensors or host arrays, or None"""
        if pair is None:
            return
        if self._acc is None:
            self.n_comp = pair[0].shape[0] + (1 if self._scores is not None else 0)
            if pair[0].shape[-1] > 0:
                assert self.n_comp * self._target.rows_out == self._vec_size
            self._acc = _acc_pool.take(self._target.fn, self._n_levels, self._target.mode, self.n_comp, mean_only=self._mean_only)
            if self._target.mode == engine.LevelAccumulator.COMPONENT_COV:
                self._acc.set_shift(self._target.shift)          # this estimate's shift (the pooled one may carry another)
        if pair[0].shape[-1] == 0:                               # empty chunk / every sample deselected
            return
        fine, coarse = pair
        if self._scores is not None:
            self._flush()
            for z_fine, z_coarse in self._scores.blocks(fine, coarse, self._dev):
                self._acc.push(level_id, z_fine, z_coarse)
            return
        if self.n_comp == 1:
            fine, coarse = fine[0], (None if coarse is None else coarse[0])
        resident = (not self._pushed_directly and getattr(fine, "is_cuda", False) and fine.is_contiguous()
                    and (coarse is None or (getattr(coarse, "is_cuda", False) and coarse.is_contiguous())))
        if resident:
            self._gathered.append((level_id, fine, coarse))
            return
        self._flush()
        self._acc.push(level_id, fine, coarse)

    def _flush(self):
        self._pushed_directly = True
        for item in self._gathered:
            self._acc.push(*item)
        self._gathered.clear()

    def finish(self, group):
        """-> n, n_rm [L], sums, sums_sq [L, K]; the accumulator goes back to the pool"""
        if self._acc is None:
            raise Exception("All samples were masked")
        if self._gathered and not self._pushed_directly:
            out = self._acc.estimate(self._gathered, group=group)
        else:
            self._flush()
            out = self._acc.finalize(group=group)
        _acc_pool.give(self._target.fn, self._n_levels, self._target.mode, self.n_comp, self._acc, mean_only=self._mean_only)
        return out


class _ConcordanceSink:
    """Where the (level, pair) stream of component_concordance ends: int64 device counters [L, ...] whose level slice
    mlmc_concordance_counts adds every pushed block to.  With scores the pair goes through _ScoreRows.uniforms block by block and
    the uniforms are counted; without, the raw rows are (a host chunk is uploaded, as the covariance route uploads it)."""

    def __init__(self, walk, M, lower, upper, scores, pairs):
        import torch
        self._dev, self._M, self._lower, self._upper = walk.dev, M, lower, upper
        L, G = walk.n_levels, lower.shape[0]
        self._scores = None if scores is None else _ScoreRows(scores, "component_concordance")
        self._pair = torch.zeros((L, G, 3, M, M), dtype=torch.int64, device=walk.dev) if pairs else None
        self._all = torch.zeros((L, G, 3), dtype=torch.int64, device=walk.dev)
        self._kept = torch.zeros((L, 1), dtype=torch.int64, device=walk.dev)
        self._seen = np.zeros(L, dtype=np.int64)
        torch.cuda.current_stream(walk.dev).synchronize()           # the zeros, before the library adds on its own stream

    def _count(self, level_id, fine, coarse, n, ld):
        from ..tool import simple_distribution
        simple_distribution._concordance_into(fine, coarse, self._M, n, ld, self._lower, self._upper,
                                              None if self._pair is None else self._pair[level_id], self._all[level_id],
                                              self._kept[level_id])

    def push(self, level_id, pair):
        import torch
        if pair is None or pair[0].shape[-1] == 0:
            return
        fine, coarse = pair
        n = int(fine.shape[-1])
        self._seen[level_id] += n
        if self._scores is not None:
            for u_fine, u_coarse in self._scores.uniforms(fine, coarse, self._dev):
                self._count(level_id, u_fine, u_coarse, u_fine.shape[-1], u_fine.shape[-1])
            return
        fine, copied = _device_rows(fine, self._M, self._dev)
        if coarse is not None:
            coarse, copied_c = _device_rows(coarse, self._M, self._dev)
            copied = copied or copied_c
        if copied:
            torch.cuda.current_stream(self._dev).synchronize()      # the library reads them on its own stream
        self._count(level_id, fine, coarse, n, n)

    def finish(self):
        """-> n, n_rm [L], pair [L, G, 3, M, M] | None, all [L, G, 3] (NumPy int64)"""
        n = self._kept.cpu().numpy()[:, 0]
        return n, self._seen - n, (None if self._pair is None else self._pair.cpu().numpy()), self._all.cpu().numpy()


ComponentConcordance = collections.namedtuple("ComponentConcordance", "n n_rm pair all")


def component_concordance(quantity, lower, upper, scores=None, pairs=True):
    """Per level, how often the scalar components of `quantity` lie inside box events -- pair by pair and all at once, fine against
    coarse (mlmc_concordance_counts, mlmc_amd/csrc/concordance.hip): the integers of a multilevel joint frequency, one pass per
    stored chunk for the whole pair matrix (concordance_statistics turns them into means and variances).

    Without `scores` the limits are in the units of the components and the raw rows are counted.  With scores = a list of M
    distributions with multipliers (one quadrature) the limits are in U SPACE: every pair goes block by block (score_block_columns(M)
    columns, one reused workspace) through the probability-integral transform u = Fhat_m(x) on the device, the bits of
    mlmc_density_cdf_batch, and the uniforms are counted without ever being downloaded.  A value that is NaN or outside its
    density's open domain has u = NaN and drops its column, like any NaN in any component, fine or coarse: so `n` equals the
    n_samples of Estimate.estimate_score_correlation on the same store.  The counts are integers: the block width changes nothing.
    :param lower, upper: limits that broadcast to [G, M]; -inf / +inf: no limit on that side; inside is lower < v < upper
    :param pairs: False: the `all` counters alone
    :return: ComponentConcordance(n [L], n_rm [L] kept and dropped samples, pair [L, G, 3, M, M] | None, all [L, G, 3]), int64; the
        axis of 3 holds the counts of the fine event, of the coarse event and of the columns where the two differ"""
    from .. import _lib
    from ..tool import simple_distribution
    M, _, scores = _component_args("component_concordance", quantity, None, scores, _lib.CONCORDANCE_MAX_M)
    lower, upper = simple_distribution._concordance_limits("component_concordance", lower, upper, M)
    with _estimate_lock:
        target = _estimate_target(quantity, True)
        walk = _walk_setup(quantity, target.source)
        sink = _ConcordanceSink(walk, M, lower, upper, scores, pairs)
        with contextlib.closing(_level_pairs(target, walk)) as level_pairs:
            for level_id, pair in level_pairs:
                sink.push(level_id, pair)
        return ComponentConcordance(*sink.finish())


def concordance_statistics(n, counts):
    """Level statistics of indicator products from their counts: counts [L, G, 3, ...] (the fine event, the coarse event, the
    columns where they differ) and n [L] kept samples.  The level difference is -1, 0 or 1, so with S = N^f - N^c and Q = N^x
    mean_l = S / n_l and var_l = (Q - S^2 / n_l) / (n_l - 1) exactly (inf where n_l <= 1: engine.level_stats).
    -> dict(l_means, l_vars [L, G, ...], prob = sum_l mean_l, var = sum_l var_l / n_l [G, ...])"""
    counts = np.asarray(counts)
    n = np.asarray(n, dtype=np.int64)
    L = counts.shape[0]
    s = (counts[:, :, 0] - counts[:, :, 1]).astype(np.float64)
    shape = s.shape[1:]
    l_means, l_vars = engine.level_stats(n, s.reshape(L, -1), counts[:, :, 2].astype(np.float64).reshape(L, -1))
    with np.errstate(all="ignore"):
        var = np.sum(l_vars / n.astype(np.float64)[:, None], axis=0)
    return dict(l_means=l_means.reshape((L,) + shape), l_vars=l_vars.reshape((L,) + shape),
                prob=np.sum(l_means, axis=0).reshape(shape), var=var.reshape(shape))


class _LikelihoodSink:
    """Where the (level, pair) stream of component_copula_likelihood ends: every pair goes block by block through
    _ScoreRows.uniforms, mlmc_copula_log_density runs on each block of device-resident uniforms, and the level sums of the blocks
    are added on the host in arrival order."""

    def __init__(self, walk, M, models, scores):
        self._dev, self._M, self._models = walk.dev, M, models
        G = models.dof.size
        self._scores = _ScoreRows(scores, "component_copula_likelihood")
        self._kept = np.zeros(walk.n_levels, dtype=np.int64)
        self._seen = np.zeros(walk.n_levels, dtype=np.int64)
        self._sums = np.zeros((walk.n_levels, 3 * G + G * G))

    def push(self, level_id, pair):
        from ..tool import simple_distribution
        if pair is None or pair[0].shape[-1] == 0:
            return
        fine, coarse = pair
        self._seen[level_id] += int(fine.shape[-1])
        for u_fine, u_coarse in self._scores.uniforms(fine, coarse, self._dev):
            nc = int(u_fine.shape[-1])
            kept, sums = simple_distribution._copula_log_density_into(self._models, u_fine, u_coarse, nc, nc)
            self._kept[level_id] += kept
            self._sums[level_id] += sums

    def finish(self):
        """-> n, n_rm [L], sum l^f, sum l^c, sum d [L, G], sum d_g d_h [L, G, G]"""
        G = self._models.dof.size
        s = self._sums
        return (self._kept, self._seen - self._kept, s[:, :G].copy(), s[:, G:2 * G].copy(), s[:, 2 * G:3 * G].copy(),
                s[:, 3 * G:].reshape(-1, G, G).copy())


ComponentCopulaLikelihood = collections.namedtuple("ComponentCopulaLikelihood", "n n_rm sum_fine sum_coarse sum_diff sum_gram models")


def component_copula_likelihood(quantity, scores, corrs, dofs):
    """Per level, the sums of the log densities of G copula models at the probability-integral transforms of the stored samples of
    the scalar components of `quantity` (mlmc_copula_log_density, mlmc_amd/csrc/copula_lik.hip): one pass per stored chunk for all
    models (tool.simple_distribution.likelihood_statistics turns the sums into means, variances and paired differences).

    Every pair goes block by block (score_block_columns(M) columns, one reused workspace) through u = Fhat_m(x) on the device, the
    bits of mlmc_density_cdf_batch, and the entry runs on each block without the uniforms ever being downloaded.  A value that is
    NaN or outside its density's open domain has u = NaN and drops its column, like any NaN in any component, fine or coarse: so
    `n` equals the n_samples of Estimate.estimate_score_correlation on the same store.  The sums of a block are a fixed tree; the
    blocks are added on the host in arrival order, so the float sums depend on the block width (`score_block_columns`) in their
    last bits.  For a given store the result repeats bit for bit.
    :param scores: a list of M distributions with multipliers (one quadrature)
    :param corrs: one correlation matrix [M, M] for all models or one per model; each goes through correlation_factor
    :param dofs: one value per model: floats in [1, 64], np.inf for the Gaussian copula
    :return: ComponentCopulaLikelihood(n [L], n_rm [L] kept and dropped samples, sum_fine, sum_coarse, sum_diff [L, G] the sums of
        l^f, l^c and d = l^f - l^c (l^c = 0 on a level without coarse values), sum_gram [L, G, G] the sums of d_g d_h, models the
        CopulaModels that were evaluated)"""
    from .. import _lib
    from ..tool import simple_distribution
    what = "component_copula_likelihood"
    if scores is None:
        raise ValueError(what + ": scores (the M marginal distributions) are required")
    M, _, scores = _component_args(what, quantity, None, scores, _lib.COPULA_LIK_MAX_M)
    models = simple_distribution._copula_models(what, corrs, dofs, M)
    with _estimate_lock:
        target = _estimate_target(quantity, True)
        walk = _walk_setup(quantity, target.source)
        sink = _LikelihoodSink(walk, M, models, scores)
        with contextlib.closing(_level_pairs(target, walk)) as level_pairs:
            for level_id, pair in level_pairs:
                sink.push(level_id, pair)
        return ComponentCopulaLikelihood(*sink.finish(), models)


def _on_device_subsample(pair, target, level_id):
    """the pair, or its share of the sub-sample of Quantity.subsample"""
    if target.subsample_params is not None and pair is not None and pair[0].shape[-1] > 0:
        return _subsample_on_device(pair, target.subsample_params[level_id])
    return pair


def _level_pairs(target, walk):
    """Generator of (level id, (fine [M, n], coarse [M, n] | None)) of an estimate, in the order in which they are pushed: the
    levels that are resident as ONE tensor, in sorted order; then the levels that the streaming feed lands as one tensor; then the
    remaining chunks in storage order, read ahead by a helper thread while this thread uploads and launches.  A level that arrives
    in several resident chunks (HDF5 files deliver levels that way) is concatenated into ONE tensor before it is handed on -- once;
    the level-wide entry replaces the chunk entries in the cache -- so every estimate, the first one included, is one push per level
    and gives bit-identical sums.  Closing the generator stops the read-ahead."""
    level_ids = {int(l) for l in walk.storage_q.level_ids()}
    done = set()
    if walk.use_cache:
        for level_id in sorted(level_ids):
            item = _device_cache.get((walk.ident, level_id, "level", walk.n_collected[level_id]))
            if item is not None:
                done.add(level_id)
                yield level_id, _on_device_subsample((item[0], item[1]), target, level_id)   # the whole level is one resident chunk
    if done >= level_ids:
        return      # (a storage that cuts its levels into hundreds of chunks: its chunk specs need not even be generated)
    specs = [cs for cs in walk.storage_q.chunks() if int(cs.level_id) not in done]
    first_raw, to_read = {}, []
    if walk.plan is not None and not hasattr(getattr(walk.plan.leaf, "_storage", None), "device_row"):
        for level_id, pair in _streamed_level_pairs(target, walk, specs, first_raw):
            done.add(level_id)
            yield level_id, pair
        specs = [cs for cs in specs if int(cs.level_id) not in done]
        to_read = _chunks_to_read(walk, specs, first_raw)
    consolidate = walk.use_cache and target.subsample_params is None
    prefetch = _ChunkPrefetcher(walk.plan.leaf, to_read) if len(to_read) > 1 else None
    waiting = {id(cs) for cs in to_read} if prefetch is not None else ()
    try:
        for level_id, level_specs in itertools.groupby(specs, key=lambda cs: int(cs.level_id)):
            level_specs, pairs = list(level_specs), []
            for chunk_spec in level_specs:
                raw = prefetch.get(chunk_spec) if id(chunk_spec) in waiting else first_raw.pop(id(chunk_spec), None)
                pair = _chunk_for_device(target.source, walk.plan, chunk_spec, walk.n_collected, walk.use_cache, raw)
                pairs.append(_on_device_subsample(pair, target, level_id))
            merged = _merge_level(pairs) if (consolidate and len(pairs) > 1) else None
            if merged is not None:
                _device_cache.put_tensors((walk.ident, level_id, "level", walk.n_collected[level_id]), merged[0], merged[1],
                                          owner=walk.owner)
                for chunk_spec in level_specs:
                    _device_cache.drop(_chunk_key(walk.ident, chunk_spec, walk.n_collected))
                pairs = [merged]
            for pair in pairs:
                yield level_id, pair
    finally:
        if prefetch is not None:
            prefetch.close()


def _streamed_level_pairs(target, walk, specs, first_raw):
    """Levels of a lowered tree that the storage hands out in several chunks of [n][2][M] records: the whole level becomes ONE
    device tensor in the storage's layout -- resident from an earlier estimate of any quantity over this storage, or streamed now
    through pinned staging blocks (_LevelStreamer) -- and the tree runs as ONE k_expr launch over it.  A first chunk that was read
    on the way for a level that does not qualify is left in `first_raw`."""
    plan, n_collected, use_cache = walk.plan, walk.n_collected, walk.use_cache
    by_level = collections.OrderedDict()
    for cs in specs:
        by_level.setdefault(int(cs.level_id), []).append(cs)
    candidates = [(level_id, level_specs) for level_id, level_specs in by_level.items()
                  if not (use_cache and any(_chunk_key(walk.ident, cs, n_collected) in _device_cache for cs in level_specs))]
    for level_id, blk in _level_blocks_on_device(plan, walk.owner, candidates, n_collected, use_cache, first_raw):
        t, sn, sw, n, width = blk
        fine, coarse, _ = plan.evaluate([t[r:] for r in plan.in_rows], has_coarse=(width == 2), n=n, sample_stride=sn,
                                        side_stride=max(sw, 1), sync=not use_cache)
        if use_cache:
            _device_cache.put_tensors((walk.ident, level_id, "level", n_collected[level_id]), fine, coarse, owner=walk.owner)
        yield level_id, _on_device_subsample((fine, coarse), target, level_id)


def _chunks_to_read(walk, specs, first_raw):
    """The chunks of a lowered tree that have to come from the host storage (neither their result rows nor their stored block are
    resident), for the read-ahead of _ChunkPrefetcher."""
    to_read = []
    if _ChunkPrefetcher.enabled():
        have, owner = _device_cache, walk.owner
        for cs in specs:
            key = _chunk_key(walk.ident, cs, walk.n_collected)
            resident = walk.use_cache and (key in have or (("block", id(owner)) + key[1:]) in have
                                           or all((("row", id(owner)) + key[1:] + (r,)) in have for r in walk.plan.in_rows))
            if not resident and id(cs) not in first_raw:
                to_read.append(cs)
    return to_read


def _estimate_mean(quantity, group, variance):
    target = _estimate_target(quantity, variance)
    walk = _walk_setup(quantity, target.source)
    fn, lin_fn, n_levels, rows_out = target.fn, target.lin_fn, walk.n_levels, target.rows_out
    memo_key = None
    if walk.n_collected is not None and target.subsample_params is None and group is None and not engine._dist_group_active(group):
        memo_key = (walk.ident, walk.n_collected, _cache_generation)
    if not variance and target.mode == engine.LevelAccumulator.MOMENTS and lin_fn is None and fn is not None:
        short = _sums_from_linearized_memo(fn, memo_key, walk.owner)
        if short is not None:
            n_samples, n_rm_samples, sums, n_comp = short
            return _finish_estimate(quantity, fn, n_levels, n_comp, rows_out, n_samples, n_rm_samples, sums,
                                    np.full_like(sums, np.nan))
    sink = _LevelSink(target, walk, quantity.size(), variance)
    with contextlib.closing(_level_pairs(target, walk)) as pairs:    # (a push that raises still stops the read-ahead thread)
        for level_id, pair in pairs:
            sink.push(level_id, pair)
    n_samples, n_rm_samples, sums, sums_sq = sink.finish(group)
    if int(np.sum(n_samples)) == 0:
        raise Exception("All samples were masked")
    if lin_fn is not None:
        if memo_key is not None:
            lin_fn.__dict__["_lin_memo"] = dict(key=memo_key, n=n_samples.copy(), n_rm=n_rm_samples.copy(), sums=sums.copy(),
                                                n_comp=sink.n_comp, K=fn.size, R=lin_fn.size, owner=_BlockMeta._ref(walk.owner))
        sums = linearize.covariance_sums_from_moment_sums(lin_fn, sums, sink.n_comp)
        sums_sq = np.full_like(sums, np.nan)                       # mean only: the variances were not asked for
        fn = lin_fn
    return _finish_estimate(quantity, fn, n_levels, sink.n_comp, rows_out, n_samples, n_rm_samples, sums, sums_sq)


BOOTSTRAP_FAMILIES = ("Legendre", "Monomial", "Fourier")     # moments families of the batched bootstrap (mlmc_bootstrap_create)


def bootstrap_sizes(seed, level, chunk, k, n_level, n_chunk, n_replicates):
    """Sub-sample sizes of one stored chunk for replicates 0 .. n_replicates - 1, as the loop draws them per chunk
    (_subsample_on_device): Hypergeometric(good = k, bad = N - k, draws = min(n_c, N)), here from a generator keyed by
    (seed, level, chunk index of the level) alone -- replicate b's size does not depend on the number of replicates."""
    rng = np.random.default_rng([int(seed), int(level), int(chunk)])
    return rng.hypergeometric(int(k), int(n_level) - int(k), min(int(n_chunk), int(n_level)), size=int(n_replicates)).astype(np.int64)


def bootstrap_stream(level, chunk):
    """Philox stream of a stored chunk (mlmc_bootstrap_weights / mlmc_bootstrap_accum): level << 20 | chunk index of the level."""
    return (int(level) << 20) | int(chunk)


def bootstrap_moments(quantity, moments_fn, n_replicates, sample_vector, seed):
    """Level sums of `moments(quantity, moments_fn, mom_at_bottom=False)` for n_replicates bootstrap sub-samples at once
    (Estimate.est_bootstrap_batch).  Replicate b picks, in stored chunk c of level l (n_c samples, N_l collected, k_l requested),
    s = bootstrap_sizes(seed, l, c, ...)[b] samples uniformly with replacement; its sums are those of estimate_mean over that
    resample.  Walks the storage's own chunks (not the consolidated level tensors); ONE device wait, at the end.
    -> n [B, L] kept counts, s, sp [B, L, M * R] (row m * R + r)"""
    with _estimate_lock:
        return _bootstrap_moments(quantity, moments_fn, n_replicates, sample_vector, seed)


def _bootstrap_moments(quantity, moments_fn, n_replicates, sample_vector, seed):
    M, walk = int(quantity.size()), _walk_setup(quantity)
    return _bootstrap_walk(quantity, walk, ("acc", id(moments_fn), M, walk.n_levels, int(n_replicates)),
                           lambda: engine.BootstrapAccumulator(moments_fn, M, walk.n_levels, n_replicates),
                           n_replicates, sample_vector, seed)


def bootstrap_component_moments(quantity, moments_fns, n_replicates, sample_vector, seed):
    """bootstrap_moments for every scalar component of `quantity` under its own moments object (Estimate.est_bootstrap_components):
    component m (row m of the chunks) uses moments_fns[m] -- its own domain, its own NaN / out-of-domain mask -- in ONE device pass
    per stored chunk for all components (engine.ComponentBootstrapAccumulator).  The chunk walk, sizes and Philox streams are those
    of bootstrap_moments, so replicate b of component m is drawn with exactly the weights of the scalar call on
    scalar_component(quantity, m).  -> n [B, L, M] kept counts, s, sp [B, L, M, R]"""
    with _estimate_lock:
        fns = list(moments_fns)
        M, R = len(fns), int(fns[0].size)
        if int(quantity.size()) != M:
            raise ValueError("bootstrap_component_moments: {} moments objects for {} components".format(M, quantity.size()))
        walk = _walk_setup(quantity)
        return _bootstrap_walk(quantity, walk, ("acc_comp", tuple(id(fn) for fn in fns), R, walk.n_levels, int(n_replicates)),
                               lambda: engine.ComponentBootstrapAccumulator(fns, R, walk.n_levels, n_replicates),
                               n_replicates, sample_vector, seed)


def bootstrap_component_covariance(quantity, n_replicates, sample_vector, seed, shift=None, scores=None):
    """Level sums of the covariance between the M scalar components of `quantity` for n_replicates bootstrap sub-samples at once
    (Estimate.est_bootstrap_component_covariance; engine.ComponentCovBootstrapAccumulator): per replicate b and level l, with
    f~ = f - shift, c~ = c - shift, n = sum w keep, s1[m] = sum w keep (f~_m - c~_m), s2[i, j] = sum w keep (f~_i f~_j - c~_i c~_j)
    (level 0: f~_m, f~_i f~_j).  The chunk walk, sizes and Philox streams are those of bootstrap_moments and
    bootstrap_component_moments, so replicate b is drawn with exactly the weights of those calls with the same seed.  A sample
    with a NaN in any component, fine or coarse, is dropped from the whole matrix.

    scores = a list of M distributions with multipliers (the checks of component_covariance(scores=...)): the rows pushed are the
    NORMAL SCORES of the chunk under these marginals (tool.simple_distribution.normal_scores); a NaN or out-of-domain value has
    the score NaN and drops the sample.  The scores of a whole chunk of n samples are computed into a workspace of 16 M n bytes
    (fine and coarse), which is released when the chunk is done (one wait for the device per chunk on this route).  No shift can
    be given with scores.
    -> n [B, L] kept counts, s1 [B, L, M], s2 [B, L, M, M] (bitwise symmetric)"""
    M, shift, scores = _component_args("bootstrap_component_covariance", quantity, shift, scores,
                                       engine.ComponentCovBootstrapAccumulator.MAX_COMPONENTS, limit_first=True)
    score_rows = None if scores is None else _ScoreRows(scores, "bootstrap_component_covariance")
    with _estimate_lock:
        walk = _walk_setup(quantity)
        return _bootstrap_walk(quantity, walk, ("acc_xcov", M, walk.n_levels, int(n_replicates)),
                               lambda: engine.ComponentCovBootstrapAccumulator(M, walk.n_levels, n_replicates),
                               n_replicates, sample_vector, seed, setup=lambda acc: acc.set_shift(shift), score_rows=score_rows)


def _bootstrap_walk(quantity, walk, key, make_acc, n_replicates, sample_vector, seed, setup=None, score_rows=None):
    """One bootstrap pass over the stored chunks of `quantity` (walk = its _walk_setup) into the pooled accumulator of the slot key[0]:
    the last call's when its key was `key`, else make_acc() replaces it (an accumulator keeps its moments objects alive, so the ids
    in a key stay unique).  setup(acc): called once before the first chunk; score_rows: a _ScoreRows whose scores of each chunk are
    accumulated in place of the chunk's own rows and released after a wait for their accumulation.  -> the accumulator's finalize()"""
    import torch
    from .. import _lib
    n_level = [int(v) for v in walk.storage_q.n_collected()]
    M = int(quantity.size())
    kept = _bootstrap_pool.pop(key[0], None)                      # the last accumulator (64 MiB of scratch, pinned size blocks)
    if kept is not None and kept[0] == key:
        acc = kept[1]
        acc.reset()
    else:
        if kept is not None:
            kept[1].close()
        acc = make_acc()
    chunk_no = collections.Counter()
    pushed = 0
    try:
        if setup is not None:
            setup(acc)
        for chunk_spec in walk.storage_q.chunks():
            level = int(chunk_spec.level_id)
            c = chunk_no[level]
            chunk_no[level] += 1
            fine, coarse = _chunk_for_device(quantity, walk.plan, chunk_spec, walk.n_collected, walk.use_cache)
            n = fine.shape[-1]
            if n == 0:
                continue
            # (a host chunk -- over the cache budget -- is uploaded, as the gather path does)
            fine, copied = _device_rows(fine, M, walk.dev)
            if coarse is not None:
                coarse, copied_c = _device_rows(coarse, M, walk.dev)
                copied = copied or copied_c
            if copied:
                torch.cuda.current_stream(walk.dev).synchronize()     # the library reads them on its own stream
            sizes = bootstrap_sizes(seed, level, c, sample_vector[level], n_level[level], n, n_replicates)
            if score_rows is not None:
                fine, coarse = score_rows.chunk(fine, coarse, n)
            acc.accum(level, fine, coarse, sizes, seed, bootstrap_stream(level, c))
            if score_rows is not None:                           # its rows are a workspace of this chunk: released once they are read
                _lib.check(_lib.lib().mlmc_synchronize())
                acc.release_last()
            pushed += 1
        if pushed == 0:
            raise Exception("All samples were masked")
        out = acc.finalize()
    except BaseException:
        acc.close()
        raise
    _bootstrap_pool[key[0]] = (key, acc)
    return out


_bootstrap_pool = {}


def bootstrap_statistics(quantity, moments_fn, n, s, sp):
    """Per-replicate l_means, l_vars, mean, var of bootstrap level sums (n [B, L], s / sp [B, L, M * R] in device row order) as
    estimate_mean(moments(quantity, moments_fn, mom_at_bottom=False)) would return them for each replicate's resample
    (engine.level_stats, QuantityMean, the 'on the surface' layout of _finish_estimate).  -> dict of arrays with a leading B axis."""
    B, L, K = s.shape
    if np.any(np.sum(n, axis=1) == 0):
        raise Exception("All samples were masked")
    node = moments(quantity, moments_fn, mom_at_bottom=False)
    n_comp = K // int(moments_fn.size)
    if n_comp > 1:
        s = s.reshape(B, L, n_comp, -1).transpose(0, 1, 3, 2).reshape(B, L, K)
        sp = sp.reshape(B, L, n_comp, -1).transpose(0, 1, 3, 2).reshape(B, L, K)
    l_means, l_vars = engine.level_stats(n.reshape(B * L), s.reshape(B * L, K), sp.reshape(B * L, K))
    l_means, l_vars = l_means.reshape(B, L, K), l_vars.reshape(B, L, K)
    mean = np.sum(l_means, axis=1)
    with np.errstate(all="ignore"):
        var = np.sum(l_vars / n[:, :, None], axis=1)
    shape = np.shape(node.qtype.reshape(np.zeros(K)))
    return dict(n_samples=np.array(n), l_means=l_means.reshape((B, L) + shape), l_vars=l_vars.reshape((B, L) + shape),
                mean=mean.reshape((B,) + shape), var=var.reshape((B,) + shape))


def _finish_estimate(quantity, fn, n_levels, n_comp, rows_per_comp, n_samples, n_rm_samples, sums, sums_sq):
    if fn is not None and not quantity._at_bottom and n_comp > 1:
        # device rows are (component, moment...); 'on the surface' wants (moment..., component)
        sums = sums.reshape(n_levels, n_comp, rows_per_comp).transpose(0, 2, 1).reshape(n_levels, -1)
        sums_sq = sums_sq.reshape(n_levels, n_comp, rows_per_comp).transpose(0, 2, 1).reshape(n_levels, -1)
    l_means, l_vars = engine.level_stats(n_samples, sums, sums_sq)
    return qmod.QuantityMean(quantity.qtype, l_means=l_means, l_vars=l_vars, n_samples=[int(v) for v in n_samples],
                             n_rm_samples=[int(v) for v in n_rm_samples])
