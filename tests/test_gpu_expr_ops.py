"""Every opcode of the quantity-expression kernels on the device against a reference (cases, references and units:
tests/expr_cases.py): the byte-code interpreter k_expr of expr.hip in its 12 instantiations (pair / level 0, 1, 2 and 4 samples
per thread, with and without the libm-backed operations) and the per-program kernels of expr_jit.hip (k_pair packed and strided,
k_single), both with the row pointers by value and through the device table.  Exact opcodes bit for bit with
lowering.run_reference, libm-backed ones against the Annex F table and mpmath, the compiled form bit for bit with the
interpreter, and a sweep over the sizes around the block and compaction boundaries with selecting programs."""
import numpy as np
import pytest

from tests import expr_cases as ec

pytestmark = pytest.mark.gpu
LAYOUTS = ("level0", "packed", "strided")
M_BLOCK = 3                      # the strided layout: a row of a stored [n, 2, M] block, sample_stride = 2 M, side_stride = M
SLOTS = (2, 1, 4)                # samples per thread of the interpreter (MLMC_EXPR_SLOTS); the first one is judged, the others equal it
ERRORS = {}                      # opcode -> (largest ulps, argument) over everything this module has judged


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


_DEVICE, _PLANS = {}, {}


def _device_rows(key, block, layout, table):
    """the stored block [3, n, 2] on the device in one layout -> the row tensors in slot order (cached: they stay alive)"""
    import torch
    got = _DEVICE.get((key, layout, table))
    if got is None:
        dev = torch.device("cuda", 0)
        if layout == "level0":
            three = [torch.from_numpy(np.array(block[r, :, 0])).to(dev) for r in range(3)]
        elif layout == "packed":
            three = [torch.from_numpy(np.array(block[r])).to(dev) for r in range(3)]
        else:
            t = torch.from_numpy(np.array(block.transpose(1, 2, 0), order="C")).to(dev)      # [n, 2, M]
            assert t.shape[2] == M_BLOCK and t.stride() == (2 * M_BLOCK, M_BLOCK, 1)
            three = [t[:, :, r] for r in range(3)]
        if table:
            rows = [three[0]] * ec.TABLE_ROWS                          # the rows no instruction loads: any valid pointer
            rows[ec.TABLE_A], rows[ec.TABLE_B], rows[ec.TABLE_X] = three
        else:
            rows = three
        torch.cuda.synchronize()
        got = _DEVICE[(key, layout, table)] = rows
    return got


def _plan(program):
    if program.name not in _PLANS:
        _PLANS[program.name] = program.plan()
    return _PLANS[program.name]


def _evaluate(plan, rows, layout, n):
    """-> [n_out, n', sides] on the host"""
    pair = layout != "level0"
    strides = dict(sample_stride=2 * M_BLOCK, side_stride=M_BLOCK) if layout == "strided" else {}
    f, c, _ = plan.evaluate([r[:n] for r in rows], has_coarse=pair, n=n, sync=True, **strides)
    got = f.cpu().numpy()[:, :, None]
    if pair:
        got = np.concatenate([got, c.cpu().numpy()[:, :, None]], axis=2)
    return got


def _host_block(block, layout, n=None):
    b = block[:, :n] if n is not None else block
    return b[:, :, :1] if layout == "level0" else b


def _check(program, block, got, tol=None):
    if program.selects:
        return ec.check_selecting(program, block, got)
    return ec.check_program(program, block, got, tol=tol, errors=ERRORS)


def _programs(op):
    built = ec.forms(op)
    tab = ec.forms(op, table=True)
    return list(built.values()) + [tab["ragged" if op == "SELECT" else "rr"]]


def _fits(program, layout, slots):
    """the condition under which mlmc_expr_eval honours MLMC_EXPR_SLOTS"""
    return program.n_regs * (1 if layout == "level0" else 2) * slots * 256 * 8 <= 65536


@pytest.mark.parametrize("family", list(ec.FAMILIES))
def test_interpreter_against_the_reference(hip, monkeypatch, family):
    """k_expr: every opcode of the family in every operand form, on level-0 rows, packed pairs and strided pairs, at 1, 2 and 4
    samples per thread; a light opcode also inside a libm-backed program, a libm-backed one alone (a hole in the `heavy` list of
    mlmc_expr_create gives zeros), the row pointers also through the device table"""
    monkeypatch.setenv("MLMC_EXPR_JIT", "0")
    for op in ec.FAMILIES[family]:
        block = ec.arguments(ec.CASES[op][0])
        n = block.shape[1]
        for program in _programs(op):
            plan = _plan(program)
            launches = plan.jit_state()[1]
            for layout in LAYOUTS:
                rows = _device_rows(ec.CASES[op][0], block, layout, program.table)
                first = None
                for slots in SLOTS:
                    assert _fits(program, layout, slots)
                    monkeypatch.setenv("MLMC_EXPR_SLOTS", str(slots))
                    got = _evaluate(plan, rows, layout, n)
                    if first is None:
                        first = got
                        _check(program, _host_block(block, layout), got)
                    else:
                        assert got.shape == first.shape and ec.same_bits(got, first).all(), (program.name, layout, slots)
            assert plan.jit_state()[1] == launches, program.name           # no compiled launch: the interpreter ran every time


@pytest.mark.parametrize("family", list(ec.FAMILIES))
def test_compiled_against_the_interpreter_and_the_reference(hip, monkeypatch, family):
    """the kernel generated for each program (k_pair packed and strided, k_single; NaN, +-inf and -0.0 immediates in both operand
    slots): it really runs, its rows equal the interpreter's bit for bit, libm-backed opcodes included, and pass the reference"""
    monkeypatch.setenv("MLMC_EXPR_JIT_VERBOSE", "1")                       # a hiprtc failure prints its log
    monkeypatch.delenv("MLMC_EXPR_SLOTS", raising=False)
    for k, op in enumerate(ec.FAMILIES[family]):
        block = ec.arguments(ec.CASES[op][0])
        n = block.shape[1]
        for program in _programs(op):
            if program.form == "in_heavy" or (program.table and k > 0):    # the compiled form knows no HEAVY; one table form a family
                continue
            plan = _plan(program)
            for layout in LAYOUTS:
                rows = _device_rows(ec.CASES[op][0], block, layout, program.table)
                monkeypatch.setenv("MLMC_EXPR_JIT", "0")
                launches = plan.jit_state()[1]
                interpreted = _evaluate(plan, rows, layout, n)
                assert plan.jit_state()[1] == launches
                monkeypatch.setenv("MLMC_EXPR_JIT", "1")
                monkeypatch.setenv("MLMC_EXPR_JIT_AFTER", "0")
                compiled = _evaluate(plan, rows, layout, n)
                assert plan.jit_state() == ("compiled", launches + 1), (program.name, layout, plan.jit_state())
                assert compiled.shape == interpreted.shape, (program.name, layout)
                same = ec.same_bits(compiled, interpreted)
                assert same.all(), (program.name, layout, np.argwhere(~same)[:4].tolist(), compiled[~same][:4], interpreted[~same][:4])
                _check(program, _host_block(block, layout), compiled)


@pytest.mark.parametrize("name", list(ec.size_programs()))
def test_sizes_and_selection(hip, monkeypatch, name):
    """n around the block (256 threads x 1, 2, 4 samples) and compaction-chunk (4096) boundaries, n = 1 included: an arithmetic
    program, a libm-backed one and three selecting ones (keep none / all / a ragged part), interpreter and compiled form, on
    level-0 rows, packed and strided pairs, and with 65 stored rows through the device table; n_selected and the order of the
    kept samples are those of run_reference"""
    monkeypatch.setenv("MLMC_EXPR_JIT_VERBOSE", "1")
    monkeypatch.setenv("MLMC_EXPR_JIT_AFTER", "0")
    monkeypatch.delenv("MLMC_EXPR_SLOTS", raising=False)
    block = ec.size_block()
    kept = []
    for table in (False, True):
        program = ec.size_programs(table)[name]
        plan = _plan(program)
        launches = plan.jit_state()[1]
        for layout in (("packed",) if table else LAYOUTS):
            rows = _device_rows("sizes", block, layout, table)
            for n in ec.SIZES:
                host = _host_block(block, layout, n)
                monkeypatch.setenv("MLMC_EXPR_JIT", "0")
                interpreted = _evaluate(plan, rows, layout, n)
                kept.append(_check(program, host, interpreted))
                assert plan.jit_state()[1] == launches
                monkeypatch.setenv("MLMC_EXPR_JIT", "1")
                compiled = _evaluate(plan, rows, layout, n)
                launches += 1
                assert plan.jit_state() == ("compiled", launches), (program.name, layout, n, plan.jit_state())
                assert compiled.shape == interpreted.shape and ec.same_bits(compiled, interpreted).all(), (program.name, layout, n)
                _check(program, host, compiled)
    if name == "select_none":
        assert set(kept) == {0}
    if name == "select_ragged":
        assert max(kept) > 400 and all(k < n for k, n in zip(kept, ec.SIZES * 4) if n > 1)


def test_fine_and_coarse_sides(hip, monkeypatch):
    """the coarse side carries the arguments in reversed order: it comes back in the coarse output and the fine side in the fine
    output, from the interpreter at 1, 2 and 4 samples per thread and from the compiled kernel, packed and strided"""
    block = ec.arguments("structure")
    n = block.shape[1]
    a, b, x = block[ec.ROW_A, :, 0], block[ec.ROW_B, :, 0], block[ec.ROW_X, :, 0]
    copy, neg = ec.forms("LOAD")["rr"], ec.forms("NEG")["rr"]
    monkeypatch.delenv("MLMC_EXPR_JIT_AFTER", raising=False)
    for layout in ("packed", "strided"):
        rows = _device_rows("structure", block, layout, False)
        for slots in SLOTS + (None,):
            monkeypatch.setenv("MLMC_EXPR_JIT", "0" if slots else "1")
            if slots:
                monkeypatch.setenv("MLMC_EXPR_SLOTS", str(slots))
            else:
                monkeypatch.setenv("MLMC_EXPR_JIT_AFTER", "0")
            got = _evaluate(_plan(copy), rows, layout, n)
            for k, want in enumerate((a, b, a, x)):                        # the outputs of the copy program: rows a, b, a, x
                assert ec.same_bits(got[k, :, 0], want).all() and ec.same_bits(got[k, :, 1], want[::-1]).all(), (layout, slots, k)
            got = _evaluate(_plan(neg), rows, layout, n)
            assert ec.same_bits(got[0, :, 0], -a).all() and ec.same_bits(got[0, :, 1], -a[::-1]).all(), (layout, slots)
        assert _plan(copy).jit_state()[0] == "compiled" and _plan(neg).jit_state()[0] == "compiled"


def test_report_observed_ulps(hip, monkeypatch):
    """prints, per libm-backed opcode, the largest error in ulps of the device (interpreter and compiled form, every operand form,
    packed pairs) and of NumPy's host libm on the same arguments, and the tolerance; then holds the device to the tolerance"""
    from mlmc_amd.quantity import lowering
    monkeypatch.delenv("MLMC_EXPR_SLOTS", raising=False)
    monkeypatch.setenv("MLMC_EXPR_JIT_AFTER", "0")
    device, host = {}, {}
    for op in ec.LIBM:
        block = ec.arguments(ec.CASES[op][0])
        for program in ec.forms(op).values():
            plan = _plan(program)
            want, _ = lowering.run_reference(program.plan_host(), block)
            ec.check_program(program, block, want, tol=np.inf, errors=host)
            for jit in ("0", "1"):
                monkeypatch.setenv("MLMC_EXPR_JIT", jit)
                got = _evaluate(plan, _device_rows(ec.CASES[op][0], block, "packed", False), "packed", block.shape[1])
                ec.check_program(program, block, got, tol=np.inf, errors=device)
    for op, seen in ERRORS.items():                                        # what the other tests of this run have judged
        if seen[0] > device[op][0]:
            device[op] = seen
    print()
    print("opcode   device ulps   host ulps   tolerance   worst device argument")
    for op in ec.LIBM:
        print("{:7s} {:12.3f} {:11.3f} {:11.0f}   {}".format(op, device[op][0], host[op][0], ec.tolerance(op), device[op][1]))
    for op in ec.LIBM:
        assert device[op][0] <= ec.tolerance(op), (op, device[op])
