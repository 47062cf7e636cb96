"""GPU tests of the ORDER in which quantity_estimate.estimate_mean hands sample pairs to the accumulator.  Every level sum is a
fixed-order device reduction, so the sequence of push / estimate / finalize calls, their levels and their widths fix the bits of
the result; the tests record that sequence on engine.LevelAccumulator and compare it with the one the walk is meant to produce:
one `estimate` over whole levels when the samples are resident, one `push` per stored chunk when they are not, fixed column
blocks on the normal-score route.

Storage: 3 levels of 96 / 48 / 24 samples of a quantity with M = 2 components, a 3-term Legendre basis."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = (96, 48, 24)
M = 2
DOMAIN = (-1.0, 1.0)
ENV = ("MLMC_HIP_DEVICE_CACHE_GB", "MLMC_HIP_DEVICE_TREE", "MLMC_HIP_STREAM_UPLOAD", "MLMC_HIP_BLOCK_UPLOAD",
       "MLMC_SCORE_BLOCK_COLUMNS", "MLMC_HIP_LINEARIZE")


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


def _levels():
    """[(fine [M, n], coarse [M, n] | None)], every value inside DOMAIN"""
    rng = np.random.default_rng(20241)
    out = []
    for l, n in enumerate(N):
        f = rng.uniform(-0.9, 0.9, size=(M, n))
        c = None if l == 0 else np.clip(f + 0.2 * 0.5 ** l * rng.standard_normal((M, n)), -0.95, 0.95)
        out.append((f, c))
    return out


@pytest.fixture(scope="module")
def levels():
    return _levels()


@pytest.fixture
def defaults(hip, monkeypatch):
    """the default routes (nothing of ENV set) and an empty device cache"""
    from mlmc_amd.quantity import quantity_estimate as qe
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    qe.device_cache_clear()
    yield monkeypatch
    qe.device_cache_clear()


class _Spy:
    """records (method, level, rows, columns) of LevelAccumulator.push, one such entry per item of .estimate and ("finalize",),
    and calls through; fail_at = k makes the k-th push raise instead"""

    def __init__(self, monkeypatch):
        from mlmc_amd import engine
        self.calls = []
        self.fail_at = None
        self.pushes = 0
        cls = engine.LevelAccumulator
        push, estimate, finalize = cls.push, cls.estimate, cls.finalize
        spy = self

        def shape(fine):
            return (1 if fine.ndim == 1 else int(fine.shape[0]), int(fine.shape[-1]))

        def spy_push(acc, level, fine, coarse=None):
            spy.pushes += 1
            if spy.fail_at == spy.pushes:
                raise RuntimeError("spy: push refused")
            spy.calls.append(("push", int(level)) + shape(fine))
            return push(acc, level, fine, coarse)

        def spy_estimate(acc, chunks, *args, **kw):
            spy.calls.extend(("estimate", int(c[0])) + shape(c[1]) for c in chunks)
            return estimate(acc, chunks, *args, **kw)

        def spy_finalize(acc, *args, **kw):
            spy.calls.append(("finalize",))
            return finalize(acc, *args, **kw)
        monkeypatch.setattr(cls, "push", spy_push)
        monkeypatch.setattr(cls, "estimate", spy_estimate)
        monkeypatch.setattr(cls, "finalize", spy_finalize)

    def take(self):
        out, self.calls = self.calls, []
        return out


def _quantity(levels, chunk_size=None):
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    from mlmc_amd.sample_storage import Memory
    spec = [QuantitySpec(name="q", unit="m", shape=(M, 1), times=[1], locations=['0'])]
    st = Memory(chunk_size=chunk_size)
    st.save_global_data(result_format=spec, level_parameters=[[0.5 * 0.2 ** l] for l in range(len(levels))])
    for l, (f, c) in enumerate(levels):
        st.set_level_samples(l, f.T, None if c is None else c.T)
    q = make_root_quantity(st, spec)['q']
    assert q.size() == M
    return st, q


def _moments(q):
    from mlmc_amd import Legendre
    from mlmc_amd.quantity import quantity_estimate as qe
    return qe.moments(q, Legendre(3, DOMAIN))


def _score_marginals():
    from tests import score_cases as sk
    return [sk.closed_distribution(sk.RATES[0], DOMAIN), sk.closed_distribution(sk.RATES[2], DOMAIN)]


def _bits(r):
    return (np.asarray(r.n_samples).tobytes(), np.asarray(r.n_rm_samples).tobytes(), r.l_means.tobytes(), r.l_vars.tobytes())


WHOLE_LEVELS = [("estimate", l, M, n) for l, n in enumerate(N)]


def test_one_chunk_per_level_resident(defaults, levels):
    """(a) resident chunks are gathered: no push, one estimate over the three levels"""
    from mlmc_amd.quantity import quantity_estimate as qe
    spy = _Spy(defaults)
    st, q = _quantity(levels)
    r = qe.estimate_mean(_moments(q))
    assert spy.take() == WHOLE_LEVELS
    assert list(r.n_samples) == list(N)


def test_chunked_levels_are_consolidated(defaults, levels):
    """(b) chunks of 32 with the cache on: every level reaches the accumulator as ONE tensor of the level's width, in the first
    estimate and in the second, and both give the same bits"""
    from mlmc_amd.quantity import quantity_estimate as qe
    spy = _Spy(defaults)
    st, q = _quantity(levels, chunk_size=32)
    node = _moments(q)
    first = qe.estimate_mean(node)
    assert spy.take() == WHOLE_LEVELS
    second = qe.estimate_mean(node)
    assert spy.take() == WHOLE_LEVELS
    assert _bits(first) == _bits(second)
    assert list(first.n_samples) == list(N)


def test_host_chunks_are_pushed_in_storage_order(defaults, levels):
    """(c) no cache, the tree evaluated on the host: one push per stored chunk in storage order, then finalize, no estimate"""
    from mlmc_amd.quantity import quantity_estimate as qe
    defaults.setenv("MLMC_HIP_DEVICE_CACHE_GB", "0")
    defaults.setenv("MLMC_HIP_DEVICE_TREE", "0")
    spy = _Spy(defaults)
    st, q = _quantity(levels, chunk_size=32)
    r = qe.estimate_mean(_moments(q))
    want = [("push", l, M, n) for l, n in ((0, 32), (0, 32), (0, 32), (1, 32), (1, 16), (2, 24))]
    assert spy.take() == want + [("finalize",)]
    assert list(r.n_samples) == list(N)


def test_score_blocks(defaults, levels):
    """(d) the normal-score route in blocks of 64 columns: M score rows and the row of ones per push, then finalize"""
    from mlmc_amd.quantity import quantity_estimate as qe
    defaults.setenv("MLMC_SCORE_BLOCK_COLUMNS", "64")
    spy = _Spy(defaults)
    st, q = _quantity(levels)
    r = qe.estimate_mean(qe.component_covariance(q, scores=_score_marginals()))
    want = [("push", l, M + 1, n) for l, n in ((0, 64), (0, 32), (1, 48), (2, 24))]
    assert spy.take() == want + [("finalize",)]
    assert list(r.n_samples) == list(N)


def test_a_push_that_raises_stops_the_read_ahead(defaults, levels):
    """(e) an exception in a push propagates, leaves no read-ahead thread behind and does not spoil the next estimate.  Pushes
    happen DURING the walk, with a _ChunkPrefetcher running, on the score route over a lowered tree without the cache (the
    host-evaluated tree of (c) has no read-ahead; resident chunks of other nodes are gathered and pushed after the walk)."""
    from mlmc_amd.quantity import quantity_estimate as qe
    defaults.setenv("MLMC_HIP_DEVICE_CACHE_GB", "0")
    spy = _Spy(defaults)
    readers = []                                                 # the read-ahead threads that were started
    init = qe._ChunkPrefetcher.__init__

    def spy_init(self, *args, **kw):
        before = set(threading.enumerate())
        init(self, *args, **kw)
        readers.extend(t for t in threading.enumerate() if t not in before and t.name == "mlmc-chunk-reader")
    defaults.setattr(qe._ChunkPrefetcher, "__init__", spy_init)
    walks, level_pairs = [], qe._level_pairs                     # the generators stay referenced: only close() can end them early
    defaults.setattr(qe, "_level_pairs", lambda *args: walks.append(level_pairs(*args)) or walks[-1])
    st, q = _quantity(levels, chunk_size=32)
    node = qe.component_covariance(q, scores=_score_marginals())
    fresh = qe.estimate_mean(node)
    want = [("push", l, M + 1, n) for l, n in ((0, 32), (0, 32), (0, 32), (1, 32), (1, 16), (2, 24))] + [("finalize",)]
    assert spy.take() == want and len(readers) == 1
    spy.pushes, spy.fail_at = 0, 2
    with pytest.raises(RuntimeError, match="spy: push refused"):
        qe.estimate_mean(node)
    assert spy.take() == want[:1] and len(readers) == 2
    assert len(walks) == 2 and walks[1].gi_frame is None         # closed by the consumer, not by losing its last reference
    for reader in readers:
        reader.join(30)                                          # (it ends with the chunk it was reading when it was closed)
    assert not [t.name for t in threading.enumerate() if t.name == "mlmc-chunk-reader"]
    spy.fail_at = None
    again = qe.estimate_mean(node)
    assert spy.take() == want
    assert _bits(again) == _bits(fresh)
