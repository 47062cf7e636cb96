"""Stream order and buffer lifetime of every entry that takes or returns device memory (run with -m gpu).

The library launches on a stream of its own; torch produces on its current stream.  tests/stream_cases.py holds the inventory
of entries and the late-input helper: inputs whose memory holds NaN until a copy queued behind a long chain of torch work has
run.  Every case checks, immediately before the entry, that the producer has NOT finished ("producer already finished" is a
failure, never a skip), so a missing wait reads NaN and the result differs from the settled one.  Results are compared bit for
bit through uint64 views.  The C contract of mlmc_set_stream / mlmc_wait_event / use_torch_stream runs in one child process,
because mlmc_set_stream gives up the library's own stream for good."""
import json
import os
import subprocess
import sys
import time

import pytest

from tests import stream_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = {r.name: r for r in sc.INVENTORY}


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


def _wait_all(hip):
    import torch
    hip.check(hip.lib().mlmc_synchronize())
    torch.cuda.synchronize()


_settled = {}


def settled(hip, name):
    """(tensors, aux, flat result, host wall time of the second call) of a row on settled inputs: computed once, shared, unchanged"""
    if name not in _settled:
        import torch
        row = ROWS[name]
        tensors, aux = row.build()
        torch.cuda.synchronize()
        row.run(tensors, sc.state_of(row, aux), sc.SETTLED)    # first call: handles, tables, compiled programs
        _wait_all(hip)
        state = sc.state_of(row, aux)
        t0 = time.perf_counter()
        result = row.run(tensors, state, sc.SETTLED)
        seconds = time.perf_counter() - t0
        _wait_all(hip)
        _settled[name] = (tensors, aux, row.flat(result), seconds)
    return _settled[name]


def _late_run(hip, name):
    """the row on late inputs queued on the CURRENT stream -> (flat result, result object)"""
    row = ROWS[name]
    tensors, aux, _, _ = settled(hip, name)
    state = sc.state_of(row, aux)
    late, pending = sc.late_like(tensors)
    result = row.run(late, state, pending)
    assert pending.checks >= 1, "the row never checked that its producer was pending"
    _wait_all(hip)
    return row.flat(result)


@pytest.mark.parametrize("name", sc.REQUIRED_ROWS)
def test_late_inputs_on_the_default_stream(hip, name):
    want = settled(hip, name)[2]
    got = _late_run(hip, name)
    assert sc.same_bits(got, want), "{}: {}".format(name, sc.first_difference(got, want))


@pytest.mark.parametrize("name", sc.REQUIRED_ROWS)
def test_late_inputs_on_a_side_stream(hip, name):
    import torch
    want = settled(hip, name)[2]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = _late_run(hip, name)
    assert sc.same_bits(got, want), "{}: {}".format(name, sc.first_difference(got, want))


@pytest.mark.parametrize("name", [n for n in sc.REQUIRED_ROWS if n not in sc.LIBRARY_STREAM_OUTPUTS])
def test_device_outputs_are_complete_for_torch(hip, name):
    """what an entry returns in device memory (or wrote into a tensor of the caller's), read at once by a torch op on the current
    stream, is what the tensor holds after mlmc_synchronize()"""
    row = ROWS[name]
    tensors, aux, _, _ = settled(hip, name)
    result = row.run(tensors, sc.state_of(row, aux), sc.SETTLED)
    outs = sc.cuda_tensors(result)
    early = [t.clone() for t in outs]
    _wait_all(hip)
    got = [t.cpu().numpy() for t in early]
    want = [t.cpu().numpy() for t in outs]
    assert sc.same_bits(got, want), "{}: {}".format(name, sc.first_difference(got, want))


def test_chain_outlasts_the_slowest_entry_tenfold(hip):
    """the producer chain takes at least ten times the host wall time of the slowest entry on settled inputs"""
    slowest = max(sc.REQUIRED_ROWS, key=lambda n: settled(hip, n)[3])
    entry_ms = settled(hip, slowest)[3] * 1e3
    chain_ms = sc.chain_gpu_ms()
    print("chain {:.1f} ms on the GPU; slowest entry {} {:.2f} ms on the host".format(chain_ms, slowest, entry_ms))
    for n in sorted(sc.REQUIRED_ROWS, key=lambda n: -settled(hip, n)[3])[:8]:
        print("  {:36s} {:8.2f} ms".format(n, settled(hip, n)[3] * 1e3))
    assert chain_ms >= 10.0 * entry_ms, (chain_ms, slowest, entry_ms)


# ---- lifetime ------------------------------------------------------------------------------------------------------------
def _allocator_reuses(template):
    """validity condition of the lifetime cases: a block of this size, freed, is what the caching allocator hands out next"""
    import torch
    t = template.clone()
    torch.cuda.synchronize()
    p = t.data_ptr()
    del t
    u = torch.full_like(template, float("nan"))
    assert u.data_ptr() == p, "the caching allocator did not hand back the freed block: the lifetime case proves nothing"


LIFETIME = {
    "moments": (lambda: sc._accum("moments"), "accum_push_moments"),
    "cov": (lambda: sc._accum("cov"), "accum_push_cov"),
    "xcov": (sc._xcov, "xcov_push"),
}


@pytest.mark.parametrize("kind", sorted(LIFETIME))
def test_pushed_chunks_outlive_the_callers_references(hip, kind):
    """push() returns before the library has read the chunk (the moments pushes are deferred into one launch at finalize): the
    caller drops every reference, allocates tensors of the same sizes and fills them with NaN.  The allocator would hand the
    chunks' memory out again (checked first, on a tensor nobody holds); finalize() still gives the settled result."""
    import torch
    make, row = LIFETIME[kind]
    tensors, _, want, _ = settled(hip, row)
    for t in tensors:
        _allocator_reuses(t)
    acc = make()
    chunks = sc._chunks([t.clone() for t in tensors])
    torch.cuda.synchronize()
    shapes = [(tuple(f.shape), None if c is None else tuple(c.shape)) for _, f, c in chunks]
    while chunks:
        l, f, c = chunks.pop(0)
        acc.push(l, f, c)
        del f, c
    poison = [torch.full(s, float("nan"), dtype=torch.float64, device="cuda") for pair in shapes for s in pair if s is not None]
    torch.cuda.synchronize()
    got = sc.flat_any(acc.finalize(reduce=False))
    del poison
    assert sc.same_bits(got, want), sc.first_difference(got, want)


@pytest.mark.parametrize("kind", ["moments", "component", "xcov"])
def test_bootstrap_chunks_outlive_the_callers_references(hip, kind):
    """the same for accum() of the three bootstrap accumulators"""
    import torch
    tensors, _, want, _ = settled(hip, "bootstrap_" + kind)
    acc = sc._boot(kind)
    sizes = sc.bootstrap_sizes()
    chunks = sc._chunks([t.clone() for t in tensors])
    torch.cuda.synchronize()
    shapes = [(tuple(f.shape), None if c is None else tuple(c.shape)) for _, f, c in chunks]
    while chunks:
        l, f, c = chunks.pop(0)
        acc.accum(l, f, c, sizes[l], sc.SEED, l)
        del f, c
    poison = [torch.full(s, float("nan"), dtype=torch.float64, device="cuda") for pair in shapes for s in pair if s is not None]
    torch.cuda.synchronize()
    got = sc.flat_any(acc.finalize())
    del poison
    assert sc.same_bits(got, want), sc.first_difference(got, want)


@pytest.mark.parametrize("kind", ["moments", "component", "xcov"])
def test_release_last_after_synchronize_frees_the_rows(hip, kind):
    """release_last() after mlmc_synchronize(): the rows of the last accum() are read, the caller may reuse them.  Here the
    allocator DOES hand their memory back (asserted: the validity condition) and it is overwritten with NaN before finalize()."""
    import torch
    tensors, _, want, _ = settled(hip, "bootstrap_" + kind)
    acc = sc._boot(kind)
    sizes = sc.bootstrap_sizes()
    chunks = sc._chunks([t.clone() for t in tensors])
    torch.cuda.synchronize()
    held = []
    while chunks:
        l, f, c = chunks.pop(0)
        acc.accum(l, f, c, sizes[l], sc.SEED, l)
        hip.check(hip.lib().mlmc_synchronize())
        acc.release_last()
        freed = sorted(t.data_ptr() for t in (f, c) if t is not None)
        shape = tuple(f.shape)
        del f, c
        again = [torch.full(shape, float("nan"), dtype=torch.float64, device="cuda") for _ in freed]
        assert sorted(u.data_ptr() for u in again) == freed, \
            "the caching allocator did not hand back the released rows: the case proves nothing"
        held += again                                           # kept: the next level must not land on them
        torch.cuda.synchronize()
    got = sc.flat_any(acc.finalize())
    assert sc.same_bits(got, want), sc.first_difference(got, want)


# ---- the C stream contract, in one child process -------------------------------------------------------------------------
CHILD = r'''
import ctypes as C, json, sys
sys.path.insert(0, %(root)r)
import numpy as np
import torch
from tests import stream_cases as sc
from mlmc_amd import _lib

steps, info = [], {}


def done(ok, failed=None, detail=None):
    print(json.dumps(dict(ok=ok, failed=failed, detail=detail, steps=steps, info=info)))
    sys.exit(0)


def step(name, cond, detail=None):
    if not cond:
        done(False, name, detail)
    steps.append(name)


def report_exception(kind, value, tb):
    print(json.dumps(dict(ok=False, failed="exception after step {!r}".format(steps[-1] if steps else None), detail=repr(value), steps=steps,
                          info=info)))


sys.excepthook = report_exception


lib = _lib.load()
for name, call in (("mlmc_set_stream", lambda: lib.mlmc_set_stream(None)), ("mlmc_wait_event", lambda: lib.mlmc_wait_event(None)),
                   ("mlmc_synchronize", lambda: lib.mlmc_synchronize())):
    rc = call()
    msg = lib.mlmc_last_error().decode()
    step("before init: " + name, rc != 0 and "mlmc_init has not been called" in msg, msg)
_lib.init(0)
rc = lib.mlmc_wait_event(None)
msg = lib.mlmc_last_error().decode()
step("mlmc_wait_event(NULL)", rc != 0 and "mlmc_wait_event" in msg, msg)

# the raw C calls: three device pushes and a packed device finalize; one evaluation of a two-row expression program
from mlmc_amd.engine import LevelAccumulator
from mlmc_amd.quantity import lowering
from mlmc_amd.quantity.quantity import make_root_quantity
from mlmc_amd.sample_storage import Memory

levels, _ = sc._levels()
L, K = len(sc.N_LEVEL), sc.M * sc.R
acc = sc._accum("moments")
st = Memory()
st.save_global_data(result_format=sc._spec(), level_parameters=[[s] for s in sc.STEPS])
for l, (f, c) in enumerate(sc.level_values()):
    st.set_level_samples(l, f.T, None if c is None else c.T)
q = make_root_quantity(st, sc._spec())['q'][1]['0']
plan = lowering.lower((q[1, 0] - 0.25) * q[0, 0])
n1 = sc.N_LEVEL[1]
pairs = [torch.stack([levels[1][m], levels[2][m]], dim=1).contiguous() for m in plan.in_rows]      # [n, 2] per stored row
torch.cuda.synchronize()


def c_calls(chunk_tensors, rows, packed, fine, coarse):
    """no host wait anywhere: the calls only enqueue"""
    _lib.check(lib.mlmc_accum_reset(acc._h))
    for l, f, c in sc._chunks(chunk_tensors):
        _lib.check(lib.mlmc_accum_push(acc._h, l, _lib.ptr(f), _lib.ptr(c), int(f.shape[-1]), _lib.DEVICE))
    _lib.check(lib.mlmc_accum_finalize_packed(acc._h, _lib.ptr(packed), _lib.DEVICE))
    table = (C.c_void_p * len(rows))(*[r.data_ptr() for r in rows])
    n_sel = C.c_int64(n1)
    _lib.check(lib.mlmc_expr_eval(plan.handle(), table, 1, n1, 2, 1, fine.data_ptr(), coarse.data_ptr(), C.byref(n_sel)))


def outputs():
    return (torch.full((2 * L + 2 * L * K,), float("nan"), dtype=torch.float64, device="cuda"),
            torch.full((plan.n_out * n1,), float("nan"), dtype=torch.float64, device="cuda"),
            torch.full((plan.n_out * n1,), float("nan"), dtype=torch.float64, device="cuda"))


outs = outputs()
torch.cuda.synchronize()
c_calls(levels, pairs, *outs)
_lib.check(lib.mlmc_synchronize())
want = [t.cpu().numpy() for t in outs]
step("settled C results are finite where they must be", np.isfinite(want[0][:2 * L]).all() and not np.isnan(want[1]).all())

# mlmc_set_stream: producers and consumer on the stream the library was given
s1 = torch.cuda.Stream()
_lib.check(lib.mlmc_set_stream(C.c_void_p(s1.cuda_stream)))
with torch.cuda.stream(s1):
    outs = outputs()
    late, pending = sc.late_like(list(levels) + pairs)
    pending.check()
    c_calls(late[:len(levels)], late[len(levels):], *outs)
    info["set_stream: producer still pending after the C calls"] = not pending.event.query()
    got = [t.clone() for t in outs]                           # a torch consumer on the same stream
s1.synchronize()
got = [t.cpu().numpy() for t in got]
step("set_stream: late inputs on the library's stream", sc.same_bits(got, want), sc.first_difference(got, want))

# mlmc_wait_event: the library on a second stream, the producer on the first
s2 = torch.cuda.Stream()
_lib.check(lib.mlmc_set_stream(C.c_void_p(s2.cuda_stream)))
with torch.cuda.stream(s1):
    outs = outputs()
    s1.synchronize()
    late, pending = sc.late_like(list(levels) + pairs)
pending.check()
_lib.check(lib.mlmc_wait_event(C.c_void_p(pending.event.cuda_event)))
c_calls(late[:len(levels)], late[len(levels):], *outs)
info["wait_event: producer still pending after the C calls"] = not pending.event.query()
with torch.cuda.stream(s2):
    got = [t.clone() for t in outs]
s2.synchronize()
got = [t.cpu().numpy() for t in got]
step("wait_event: late inputs on another stream", sc.same_bits(got, want), sc.first_difference(got, want))
s1.synchronize()

# use_torch_stream(): the library shares ONE torch stream; an entry called under another stream is still ordered
rows = {r.name: r for r in sc.INVENTORY}
# (four other streams: streams share a few hardware queues, and two streams on one queue run in order by accident)
s3, others = torch.cuda.Stream(), [torch.cuda.Stream() for _ in range(4)]
with torch.cuda.stream(s3):
    _lib.use_torch_stream()
_lib._on_torch_stream = True                                  # as LevelAccumulator._packed_buffer leaves it
for name in ("row_percentiles", "percentiles", "accum_estimate_moments", "normal_scores"):
    row = rows[name]
    tensors, aux = row.build()
    torch.cuda.synchronize()
    ref = row.flat(row.run(tensors, sc.state_of(row, aux), sc.SETTLED))
    for label, stream in [("another stream {}".format(i), o) for i, o in enumerate(others)] + [("the shared stream", s3)]:
        with torch.cuda.stream(stream):
            state = sc.state_of(row, aux)
            late, pending = sc.late_like(tensors)
            result = row.run(late, state, pending)
            _lib.check(lib.mlmc_synchronize())
            stream.synchronize()
            res = row.flat(result)
        step("use_torch_stream: {} under {}".format(name, label), pending.checks >= 1 and sc.same_bits(res, ref),
             sc.first_difference(res, ref))
torch.cuda.synchronize()
done(True)
'''


def test_c_stream_contract_in_a_child_process(tmp_path):
    """mlmc_set_stream, mlmc_wait_event, use_torch_stream and their errors: one child, stopped at the first failed step"""
    script = tmp_path / "stream_contract_child.py"
    script.write_text(CHILD % dict(root=ROOT))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=240, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    report = json.loads(lines[-1])
    assert report["ok"], "step {!r} failed: {} (passed: {})".format(report["failed"], report["detail"], report["steps"])
    assert r.returncode == 0, r.stderr[-3000:]
    expected = ["before init: mlmc_set_stream", "before init: mlmc_wait_event", "before init: mlmc_synchronize", "mlmc_wait_event(NULL)",
                "settled C results are finite where they must be", "set_stream: late inputs on the library's stream",
                "wait_event: late inputs on another stream"]
    expected += ["use_torch_stream: {} under {}".format(n, s) for n in ("row_percentiles", "percentiles", "accum_estimate_moments",
                                                                        "normal_scores")
                 for s in ["another stream {}".format(i) for i in range(4)] + ["the shared stream"]]
    assert report["steps"] == expected
