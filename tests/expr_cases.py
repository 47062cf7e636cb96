"""The quantity-expression kernels (include/mlmc_hip.h: mlmc_expr_create / mlmc_expr_eval; the byte-code interpreter k_expr of
mlmc_amd/csrc/expr.hip and the per-program kernels of mlmc_amd/csrc/expr_jit.hip) opcode by opcode, shared by
tests/test_expr_cases_cpu.py and tests/test_gpu_expr_ops.py.  Nothing here touches the device.

  * hand-written programs of ONE opcode in every operand form of the ABI (register-register, immediate in either slot, the
    chained *_PREV / NO_WB forms, a light opcode inside a libm-backed program, the row pointers through the device table)
  * deterministic fp64 argument sets with the edges where libm implementations go wrong, the coarse side in reversed order
  * references: lowering.run_reference (NumPy) bit for bit for the exact opcodes, mpmath at 50 digits for the libm-backed ones,
    and the special results of C Annex F written out as a table
  * the units of the comparison and the largest errors observed"""
import math

import mpmath
import numpy as np

from mlmc_amd.quantity import lowering
from tests import joint_sample_cases as jc

OP = lowering.OP
IMM_A, IMM_B, A_PREV, B_PREV, NO_WB = lowering.IMM_A, lowering.IMM_B, lowering.A_PREV, lowering.B_PREV, lowering.NO_WB
LD = np.longdouble
MP_DIGITS = 50
DBL_MAX = float(np.finfo(np.float64).max)
DBL_MIN = float(np.finfo(np.float64).tiny)
SUB_MIN = 5e-324
assert np.finfo(LD).nmant >= 63          # the references are carried in 64-bit mantissas: 2^-11 ulp of fp64

# ---- the opcodes -----------------------------------------------------------------------------------------------------------
STRUCTURE = ("LOAD", "CONST", "STORE", "SELECT")
BINARY = ("ADD", "SUB", "MUL", "DIV", "MOD", "POW", "MAXIMUM", "MINIMUM", "FMAX", "FMIN", "ATAN2", "HYPOT", "FMOD")
UNARY = ("NEG", "ABS", "SQRT", "SQUARE", "RECIP", "EXP", "EXP2", "EXPM1", "LOG", "LOG2", "LOG10", "LOG1P", "SIN", "COS", "TAN",
         "ASIN", "ACOS", "ATAN", "SINH", "COSH", "TANH", "FLOOR", "CEIL", "TRUNC", "RINT", "SIGN", "CBRT", "NOT")
COMPARE = ("LT", "LE", "GT", "GE", "EQ", "NE")
LOGIC2 = ("AND", "OR", "XOR")
# libm-backed: an error bound in ulps against mpmath, special results from the Annex F table
LIBM = ("POW", "ATAN2", "HYPOT", "EXP", "EXP2", "EXPM1", "LOG", "LOG2", "LOG10", "LOG1P", "SIN", "COS", "TAN", "ASIN", "ACOS",
        "ATAN", "SINH", "COSH", "TANH", "CBRT")
# the opcodes that need k_expr<.., HEAVY = true>: the `heavy` list of mlmc_expr_create (MOD and FMOD call fmod, which is exact)
HEAVY = frozenset(LIBM) | {"MOD", "FMOD"}
MINMAX = ("MAXIMUM", "MINIMUM", "FMAX", "FMIN")
# one entry per opcode: (operand kind, reference kind)
CASES = {}
for _n in STRUCTURE:
    CASES[_n] = ("structure", "exact")
for _n in BINARY + COMPARE + LOGIC2:
    CASES[_n] = ("binary", "libm" if _n in LIBM else ("minmax" if _n in MINMAX else "exact"))
for _n in UNARY:
    CASES[_n] = ("unary", "libm" if _n in LIBM else "exact")

FAMILIES = {
    "structure": STRUCTURE,
    "arithmetic": ("ADD", "SUB", "MUL", "DIV", "NEG", "ABS", "SQRT", "SQUARE", "RECIP"),
    "rounding": ("FLOOR", "CEIL", "TRUNC", "RINT", "SIGN"),
    "minmax": MINMAX,
    "remainder": ("MOD", "FMOD"),
    "compare": COMPARE,
    "logic": LOGIC2 + ("NOT",),
    "exponential": ("EXP", "EXP2", "EXPM1"),
    "logarithm": ("LOG", "LOG2", "LOG10", "LOG1P"),
    "trigonometric": ("SIN", "COS", "TAN"),
    "inverse_trigonometric": ("ASIN", "ACOS", "ATAN", "ATAN2"),
    "hyperbolic": ("SINH", "COSH", "TANH"),
    "power": ("POW", "HYPOT", "CBRT"),
}

# The largest device error per libm-backed opcode in ulps of the mpmath reference (units: `ulps` below), MI355X, ROCm device
# library, measured 2026-10-21 over every program form and input layout of tests/test_gpu_expr_ops.py, which prints the figures
# (-s) next to those of NumPy's host libm.  The comment names the worst argument.  The tolerance of an opcode is
# joint_sample_cases.tolerance(observed): 4 x observed rounded up to a power of two.
OBSERVED = {
    "POW": 1.043,      # pow(3.9549335927490077, 7.0)
    "ATAN2": 1.248,    # atan2(-1.6559670496629058, 1.1241989899851998)
    "HYPOT": 0.960,    # hypot(1.5, -2.4686095279302176)
    "EXP": 0.701,      # 400.37691675916835
    "EXP2": 0.716,     # 603.4367645439227
    "EXPM1": 1.344,    # 0.35202904912731947
    "LOG": 0.613,      # 1.0623915052400088
    "LOG2": 0.578,     # 0.799445761481425
    "LOG10": 0.522,    # 0.626364321466014
    "LOG1P": 1.000,    # 5e-324: the smallest subnormal comes back as 0
    "SIN": 0.659,      # -2.4435932784948473e+199
    "COS": 0.614,      # 2.5995418589239203e+236
    "TAN": 0.674,      # 2.5
    "ASIN": 0.594,     # -0.10937506587424206
    "ACOS": 0.633,     # -0.8231556938993778
    "ATAN": 1.260,     # 1.5000000000000002
    "SINH": 0.528,     # -0.6010427079923231
    "COSH": 0.508,     # -99.19912030532973
    "TANH": 0.544,     # -0.15196757193800803
    "CBRT": 0.497,     # -297.20604283677574
}
# NumPy's host libm on the same arguments stays below 1 ulp for every opcode (tests/test_expr_cases_cpu.py holds it to that):
# tanh 0.967, atan2 0.725, cosh 0.716, acos 0.710 are its worst; the device is the less accurate one for pow, atan2, hypot,
# expm1, log1p and atan, and nowhere beyond 1.4 ulps.
HOST_ULPS = 1.0


def tolerance(op):
    return jc.tolerance(OBSERVED[op])


# ---- arguments -------------------------------------------------------------------------------------------------------------
IMMEDIATES = (0.0, -0.0, 1.0, 0.5, 2.0, -3.0, 1.0 / 3.0, 1e300, math.inf, math.nan)
UNARY_MAGNITUDES = (0.0, SUB_MIN, DBL_MIN, 1e-300, 1e-20, 2.0 ** -27, 1e-8, 0.1, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 7.0, 10.0,
                    math.pi / 4, math.pi / 2, math.pi, 2 * math.pi, 22.0, 37.0, 100.0,
                    709.0, 709.782712893384, 710.0, 745.0, 1e5, 2.0 ** 53, 1e22, 1e300, DBL_MAX)
ROW_A, ROW_B, ROW_X = 0, 1, 2    # stored rows of every argument block: operand a, operand b, the argument of the companion EXP
TABLE_ROWS = 65                  # the device-table variant declares 65 stored rows and reads these three of them
TABLE_A, TABLE_B, TABLE_X = 0, 64, 33


def unary_arguments():
    """[n] 1061 values: the listed magnitudes and their two neighbours, seeded random magnitudes, both signs, NaN, +-inf.  More
    than 1024, so that even four samples per thread (a block of 1024) need a second, ragged block."""
    mags = []
    for m in UNARY_MAGNITUDES:
        mags.append(m)
        if m > 0.0:
            mags.append(float(np.nextafter(m, 0.0)))
            if m < DBL_MAX:                                             # upward from DBL_MAX is inf, which the list has
                mags.append(float(np.nextafter(m, np.inf)))
    rng = np.random.default_rng(20261021)
    mags += list(10.0 ** rng.uniform(-300.0, 300.0, 180))
    mags += list(rng.uniform(0.0, 4.0, 180))
    mags += list(rng.uniform(0.0, 800.0, 76))
    mags = np.array(mags, dtype=np.float64)
    return np.concatenate([mags, -mags, [np.nan, np.inf, -np.inf]])


def binary_values():
    """about 60 values whose outer product is the argument set of the two-operand opcodes"""
    rng = np.random.default_rng(20261022)
    vals = [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 4.0, 7.0, -7.0, 10.0, 0.5, -0.5, 1.0 / 3.0, -1.0 / 3.0,
            1.5, -1.5, 2.5, -2.5, 0.1, SUB_MIN, -SUB_MIN, 3 * SUB_MIN, DBL_MIN, -DBL_MIN, 1e-300, -1e-300, 1e-20, 1e200, -1e200,
            1e300, -1e300, DBL_MAX, -DBL_MAX, 2.0 ** 53, 2.0 ** 53 + 2.0, 1e22, float(np.nextafter(1.0, 2.0)),
            float(np.nextafter(1.0, 0.0)), -float(np.nextafter(1.0, 2.0)), 709.5, -745.5, 1023.0, -1074.0]
    vals += list(rng.normal(0.0, 3.0, 12))
    return np.array(vals, dtype=np.float64)


def _block(a, b):
    """[3, n, 2]: rows a, b and the companion argument; the coarse side carries every row in reversed order"""
    n = a.size
    x = np.random.default_rng(20261023).uniform(-2.0, 2.0, n)
    fine = np.stack([a, b, x])
    return np.ascontiguousarray(np.stack([fine, fine[:, ::-1]], axis=2))


_BLOCKS = {}


def arguments(kind):
    """the stored block [3, n, 2] of an operand kind ("unary" | "binary" | "structure")"""
    if kind not in _BLOCKS:
        if kind == "unary":
            a = unary_arguments()
            _BLOCKS[kind] = _block(a, np.roll(a, 7))
        else:
            v = binary_values()
            a, b = np.meshgrid(v, v, indexing="ij")
            _BLOCKS["binary"] = _BLOCKS["structure"] = _block(a.ravel(), b.ravel())
        _BLOCKS[kind].setflags(write=False)
    return _BLOCKS[kind]


def table_block(stored):
    """the same rows placed among 65 stored rows, for the programs built with table=True"""
    out = np.zeros((TABLE_ROWS,) + stored.shape[1:])
    out[TABLE_A], out[TABLE_B], out[TABLE_X] = stored[ROW_A], stored[ROW_B], stored[ROW_X]
    return out


# ---- programs --------------------------------------------------------------------------------------------------------------
class Program:
    """One hand-written program.  outputs[k] = (opcode name, operand a, operand b) says what result row k holds; an operand is
    ("row", ROW_*), ("imm", value) or None.  ("EXACT", None, None) is a row of several exact opcodes: run_reference bit for bit."""

    def __init__(self, op, form, prog, n_regs, outputs, table=False, selects=False):
        self.op, self.form, self.prog, self.n_regs, self.outputs = op, form, list(prog), n_regs, list(outputs)
        self.table, self.selects = table, selects
        self.in_rows = list(range(TABLE_ROWS if table else 3))
        self.name = "{}.{}{}".format(op, form, ".table" if table else "")

    @property
    def n_out(self):
        return len(self.outputs)

    def plan(self):
        return lowering.DevicePlan(None, self.in_rows, self.n_out, self.prog, self.n_regs, self.selects)

    def stored(self, block):
        return table_block(block) if self.table else block

    def plan_host(self):
        """what lowering.run_reference reads of a plan, without a device handle"""
        return _HostPlan(self)

    def operand(self, spec, block):
        """the values [n, s] of an operand of `outputs` on a stored block [3, n, s]"""
        if spec is None:
            return None
        return block[spec[1]] if spec[0] == "row" else np.full(block.shape[1:], spec[1])


def _i(name, dst=0, a=0, b=0, imm=0.0, flags=0):
    return (OP[name] | flags, dst, a, b, float(imm))


def _companion(rx, out):
    """an unrelated EXP of another row, stored to a further output row: the program needs k_expr<.., HEAVY = true>"""
    return [_i("LOAD", 0, rx, flags=NO_WB), _i("EXP", flags=A_PREV | NO_WB), _i("STORE", a=0, b=out, flags=A_PREV)]


def forms(op, table=False):
    """the programs of one opcode: {form name: Program}"""
    kind = CASES[op][0]
    ra, rb, rx = (TABLE_A, TABLE_B, TABLE_X) if table else (ROW_A, ROW_B, ROW_X)
    A, B, X = ("row", ROW_A), ("row", ROW_B), ("row", ROW_X)
    out = {}

    def add(form, prog, n_regs, outputs, selects=False):
        out[form] = Program(op, form, prog, n_regs, outputs, table, selects)

    if op in ("LOAD", "STORE"):
        # a register stored twice, a chained store, a register that outlives another load
        add("rr", [_i("LOAD", 0, ra), _i("STORE", a=0, b=2), _i("LOAD", 1, rx), _i("STORE", a=0, b=0), _i("LOAD", 0, rb, flags=NO_WB),
                   _i("STORE", b=1, flags=A_PREV), _i("STORE", a=1, b=3)], 2, [("LOAD", A, None), ("LOAD", B, None), ("LOAD", A, None),
                                                                                  ("LOAD", X, None)])
    elif op == "CONST":
        prog, outputs = [], []
        for k, c in enumerate(IMMEDIATES):
            prog += [_i("CONST", imm=c, flags=NO_WB), _i("STORE", b=k, flags=A_PREV)]
            outputs.append(("CONST", ("imm", c), None))
        k = len(IMMEDIATES)
        prog += [_i("CONST", 1, imm=-0.0), _i("CONST", 0, imm=math.nan), _i("STORE", a=1, b=k), _i("STORE", a=0, b=k + 1)]
        outputs += [("CONST", ("imm", -0.0), None), ("CONST", ("imm", math.nan), None)]
        add("rr", prog, 2, outputs)
    elif op == "SELECT":
        # keep none, keep all, keep a ragged part; the flag from a register and chained
        for form, cmp_op, thr in (("none", "LT", -math.inf), ("all", "NE", math.inf), ("ragged", "GT", 0.4)):
            add(form, [_i("LOAD", 0, rx), _i("LOAD", 1, ra), _i(cmp_op, 2, a=0, imm=thr, flags=IMM_B), _i("SELECT", a=2),
                       _i("STORE", a=0, b=0), _i("STORE", a=1, b=1)], 3, [("LOAD", X, None), ("LOAD", A, None)], selects=True)
        add("chain", [_i("LOAD", 1, ra), _i("LOAD", 0, rx), _i("GT", a=0, imm=0.4, flags=IMM_B | A_PREV | NO_WB), _i("SELECT", flags=A_PREV),
                      _i("STORE", a=0, b=0), _i("STORE", a=1, b=1)], 2, [("LOAD", X, None), ("LOAD", A, None)], selects=True)
    elif kind == "unary":
        add("rr", [_i("LOAD", 0, ra), _i(op, 1, a=0), _i("STORE", a=1, b=0)], 2, [(op, A, None)])
        add("chain", [_i("LOAD", 0, ra, flags=NO_WB), _i(op, flags=A_PREV | NO_WB), _i("STORE", b=0, flags=A_PREV),
                      _i("LOAD", 0, ra), _i(op, 1, flags=A_PREV), _i("STORE", a=1, b=1)], 2, [(op, A, None), (op, A, None)])
        if op not in HEAVY:
            add("in_heavy", [_i("LOAD", 0, ra), _i(op, 1, a=0), _i("STORE", a=1, b=0)] + _companion(rx, 1), 2,
                [(op, A, None), ("EXP", X, None)])
    else:
        add("rr", [_i("LOAD", 0, ra), _i("LOAD", 1, rb), _i(op, 2, a=0, b=1), _i("STORE", a=2, b=0)], 3, [(op, A, B)])
        add("chain", [_i("LOAD", 1, rb), _i("LOAD", 0, ra, flags=NO_WB), _i(op, b=1, flags=A_PREV | NO_WB), _i("STORE", b=0, flags=A_PREV),
                      _i("LOAD", 0, ra), _i("LOAD", 0, rb, flags=NO_WB), _i(op, a=0, flags=B_PREV | NO_WB), _i("STORE", b=1, flags=A_PREV),
                      _i("LOAD", 1, rb), _i("LOAD", 0, ra), _i(op, 2, b=1, flags=A_PREV), _i("STORE", a=2, b=2)], 3, [(op, A, B)] * 3)
        if op in lowering._IMM_OK:
            pa, pb = [_i("LOAD", 0, ra)], [_i("LOAD", 0, ra)]
            for k, c in enumerate(IMMEDIATES):
                chained = B_PREV if k == 0 else 0              # the first one takes the loaded row from the latest result
                pa += [_i(op, b=0, imm=c, flags=IMM_A | NO_WB | chained), _i("STORE", b=k, flags=A_PREV)]
                pb += [_i(op, a=0, imm=c, flags=IMM_B | NO_WB | (A_PREV if k == 0 else 0)), _i("STORE", b=k, flags=A_PREV)]
            add("imm_a", pa, 1, [(op, ("imm", c), A) for c in IMMEDIATES])
            add("imm_b", pb, 1, [(op, A, ("imm", c)) for c in IMMEDIATES])
        if op not in HEAVY:
            add("in_heavy", [_i("LOAD", 0, ra), _i("LOAD", 1, rb), _i(op, 2, a=0, b=1), _i("STORE", a=2, b=0)] + _companion(rx, 1), 3,
                [(op, A, B), ("EXP", X, None)])
    return out


def size_programs(table=False):
    """the programs of the size sweep: {name: Program}: one of exact arithmetic in every operand form, one libm-backed (an exact
    fmod row and an exp row), and the selecting programs"""
    ra, rb, rx = (TABLE_A, TABLE_B, TABLE_X) if table else (ROW_A, ROW_B, ROW_X)
    X = ("row", ROW_X)
    out = {}
    out["arithmetic"] = Program("ADD", "sizes", [
        _i("LOAD", 0, ra), _i("LOAD", 1, rb), _i("MUL", 2, a=0, b=1), _i("ADD", imm=0.5, flags=IMM_B | A_PREV | NO_WB),
        _i("SUB", 2, a=2, flags=B_PREV), _i("STORE", b=0, flags=A_PREV), _i("DIV", b=1, imm=3.0, flags=IMM_A | NO_WB),
        _i("MAXIMUM", 0, b=0, flags=A_PREV), _i("STORE", a=0, b=1), _i("ABS", a=2, flags=NO_WB), _i("SQRT", 1, flags=A_PREV),
        _i("STORE", a=1, b=2)], 3, [("EXACT", None, None)] * 3, table)
    out["heavy"] = Program("FMOD", "sizes", [
        _i("LOAD", 0, ra), _i("LOAD", 1, rb), _i("FMOD", 2, a=0, b=1), _i("STORE", a=2, b=0)] + _companion(rx, 1), 3,
        [("FMOD", ("row", ROW_A), ("row", ROW_B)), ("EXP", X, None)], table)
    sel = forms("SELECT", table)
    for form in ("none", "all", "ragged"):
        out["select_" + form] = sel[form]
    return out


SIZES = (1, 255, 256, 257, 511, 513, 1023, 1025, 4095, 4097)


def size_block():
    """[3, 4097, 2] seeded normals, the two sides independent; a size n of the sweep evaluates the first n samples"""
    blk = np.random.default_rng(20261024).normal(0.0, 1.0, (3, max(SIZES), 2))
    blk.setflags(write=False)
    return blk


def all_programs():
    """every program of every opcode, by-value rows; and the rr form of every opcode through the device table"""
    out = []
    for op in lowering._OP_NAMES:
        out += list(forms(op).values())
        tab = forms(op, table=True)
        out.append(tab["ragged" if op == "SELECT" else "rr"])
    return out


def validate(prog, n_regs, n_in_rows, n_out_rows):
    """The validation of mlmc_expr_create restated: raises AssertionError where it would refuse the program.
    -> (selects, heavy) as the library derives them"""
    assert 1 <= len(prog) <= lowering.MAX_INSTR and 1 <= n_regs <= lowering.MAX_REGS and n_in_rows >= 1 and n_out_rows >= 1
    selects = heavy = produced = False
    written, stored = [False] * n_regs, [False] * n_out_rows
    names = lowering._OP_NAMES
    for word, dst, a, b, imm in prog:
        imm_a, imm_b, prev_a, prev_b, no_wb = (bool(word & f) for f in (IMM_A, IMM_B, A_PREV, B_PREV, NO_WB))
        assert word & ~(lowering.OP_MASK | IMM_A | IMM_B | A_PREV | B_PREV | NO_WB) == 0
        code = word & lowering.OP_MASK
        assert code < len(names), "unknown opcode"
        op = names[code]
        two_operands = OP["ADD"] <= code <= OP["FMOD"] or OP["LT"] <= code <= OP["NE"]
        assert not ((imm_a or imm_b) and (not two_operands or (imm_a and imm_b))), "immediate operands"
        uses_a = op not in ("LOAD", "CONST") and not imm_a
        uses_b = (two_operands or op in LOGIC2) and not imm_b
        produces = op not in ("STORE", "SELECT")
        assert not ((prev_a and not uses_a) or (prev_b and not uses_b) or ((prev_a or prev_b) and not produced)), "chained operand"
        assert not (no_wb and not produces), "write-back"
        if produces:
            produced = True
        if op == "LOAD":
            assert a < n_in_rows, "input row"
        if uses_a and not prev_a:
            assert a < n_regs and written[a], "operand a reads an unset register"
        if uses_b and not prev_b:
            assert b < n_regs and written[b], "operand b reads an unset register"
        if op == "STORE":
            assert b < n_out_rows, "output row"
            stored[b] = True
        if produces and not no_wb:
            assert dst < n_regs, "destination register"
            written[dst] = True
        selects = selects or op == "SELECT"
        heavy = heavy or op in HEAVY
    assert all(stored), "an output row is never stored"
    return selects, heavy


def heavy_list_of_source(text):
    """the opcodes of the `heavy` switch of mlmc_expr_create in the text of expr.hip"""
    import re
    body = text[text.index("int mlmc_expr_create("):]
    body = body[body.index("switch (in.op)"):]
    body = body[:body.index("heavy = true")]
    return set(re.findall(r"case MLMC_X_([A-Z0-9]+):", body))


# ---- the exact opcodes -----------------------------------------------------------------------------------------------------
def host_apply(op, a, b):
    """NumPy's own function of an opcode on operand arrays [n, s] (the table of lowering.run_reference); comparisons follow the
    pair rule: both sides must pass"""
    table2 = {v: k for k, v in reversed(list(lowering._UFUNCS2.items()))}
    table1 = {v: k for k, v in reversed(list(lowering._UFUNCS1.items()))}
    with np.errstate(all="ignore"):
        if op in ("LOAD", "CONST"):
            return np.array(a, dtype=np.float64)
        if op in COMPARE:
            f = {"LT": a < b, "LE": a <= b, "GT": a > b, "GE": a >= b, "EQ": a == b, "NE": a != b}[op].all(axis=1)
            return np.repeat(f[:, None].astype(np.float64), a.shape[1], axis=1)
        if op in LOGIC2:
            return {"AND": np.logical_and, "OR": np.logical_or, "XOR": np.logical_xor}[op](a != 0, b != 0).astype(np.float64)
        if op == "NOT":
            return (a == 0).astype(np.float64)
        return table2[op](a, b) if op in table2 else table1[op](a)


def minmax_expected(op, a, b):
    """np_maximum / np_minimum of expr.hip restated ((a >= b || a != a) ? a : b), which fixes the zero of (+0, -0) that NumPy
    leaves to its SIMD path; FMAX / FMIN from NumPy, where two zeros may give either zero (`same_bits` is told so)"""
    with np.errstate(all="ignore"):
        if op == "MAXIMUM":
            return np.where((a >= b) | (a != a), a, b)
        if op == "MINIMUM":
            return np.where((a <= b) | (a != a), a, b)
        return (np.fmax if op == "FMAX" else np.fmin)(a, b)


def same_bits(got, want, either_zero=None):
    """[...] bool: equal including the sign of a zero; NaN equals NaN whatever its sign and payload.  either_zero: mask of the
    values where a zero of either sign passes"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    same = (got == want) & (np.signbit(got) == np.signbit(want))
    if either_zero is not None:
        same |= either_zero & (got == 0) & (want == 0)
    return same | (np.isnan(got) & np.isnan(want))


# ---- the libm-backed opcodes: C Annex F and mpmath -------------------------------------------------------------------------
def _is_int(y):
    return math.isfinite(y) and y == math.floor(y)


def _is_odd(y):
    return _is_int(y) and abs(y) < 2.0 ** 53 and int(y) % 2 == 1


def annex_f(op, a, b=None):
    """The special results of C Annex F (F.10) as an fp64 value, or None where the result is an ordinary number that the
    mpmath reference gives.  NaN stands for a domain error as well as for a NaN argument."""
    nan, inf = math.nan, math.inf
    if op == "POW":
        x, y = a, b
        if y == 0.0 or x == 1.0:
            return 1.0                                                  # even for a NaN
        if x != x or y != y:
            return nan
        if x == 0.0:
            if y < 0.0:
                return math.copysign(inf, x) if _is_odd(y) else inf
            return x if _is_odd(y) else 0.0
        if math.isinf(y):
            if x == -1.0:
                return 1.0
            return (inf if abs(x) < 1.0 else 0.0) if y < 0.0 else (0.0 if abs(x) < 1.0 else inf)
        if x == -inf:
            if y < 0.0:
                return -0.0 if _is_odd(y) else 0.0
            return -inf if _is_odd(y) else inf
        if x == inf:
            return 0.0 if y < 0.0 else inf
        if x < 0.0 and not _is_int(y):
            return nan
        return None
    if op == "ATAN2":
        y, x = a, b
        if x != x or y != y:
            return nan
        if y == 0.0 and (x > 0.0 or (x == 0.0 and not math.copysign(1.0, x) < 0.0)):
            return y                                                    # +-0 for x > 0 or +0; +-pi otherwise (a number)
        if math.isfinite(y) and y != 0.0 and x == inf:
            return math.copysign(0.0, y)
        return None
    if op == "HYPOT":
        if math.isinf(a) or math.isinf(b):
            return inf                                                  # even for a NaN
        if a != a or b != b:
            return nan
        if a == 0.0 and b == 0.0:
            return 0.0
        return None
    x = a
    if x != x:
        return nan
    zero, infinite = x == 0.0, math.isinf(x)
    if op in ("EXP", "EXP2"):
        return (inf if x > 0 else 0.0) if infinite else None
    if op == "EXPM1":
        return x if zero else ((inf if x > 0 else -1.0) if infinite else None)
    if op in ("LOG", "LOG2", "LOG10"):
        if zero:
            return -inf
        if x < 0.0:
            return nan
        return inf if infinite else (0.0 if x == 1.0 else None)
    if op == "LOG1P":
        if zero:
            return x
        if x <= -1.0:
            return -inf if x == -1.0 else nan
        return inf if infinite else None
    if op in ("SIN", "TAN"):
        return x if zero else (nan if infinite else None)
    if op == "COS":
        return nan if infinite else None
    if op == "ASIN":
        return x if zero else (nan if abs(x) > 1.0 else None)
    if op == "ACOS":
        return nan if abs(x) > 1.0 else (0.0 if x == 1.0 else None)
    if op == "ATAN":
        return x if zero else None
    if op in ("SINH", "CBRT"):
        return x if (zero or infinite) else None
    if op == "COSH":
        return inf if infinite else None
    if op == "TANH":
        return x if zero else (math.copysign(1.0, x) if infinite else None)
    raise KeyError(op)


_HUGE = 20000                    # binary exponent that stands for "far beyond fp64" in either direction


def mp_value(op, a, b=None):
    """the exact result at 50 digits of an argument for which annex_f gives None; results far beyond the range of fp64 are
    replaced by 2^+-20000 of the right sign"""
    mp = mpmath
    huge, tiny = mp.ldexp(1, _HUGE), mp.ldexp(1, -_HUGE)
    if op == "POW":
        x, y = mp.mpf(a), mp.mpf(b)
        sign = -1 if (a < 0.0 and _is_odd(b)) else 1
        L = y * mp.log(abs(x))
        return sign * (huge if L > 12000 else (tiny if L < -12000 else mp.exp(L)))
    if op == "ATAN2":
        y, x = a, b
        if math.isinf(y) or math.isinf(x) or y == 0.0 or x == 0.0:
            s = math.copysign(1.0, y)
            if math.isinf(y):
                q = mp.pi / 2 if math.isfinite(x) else (mp.pi / 4 if x > 0 else 3 * mp.pi / 4)
            elif y == 0.0 or x == -math.inf:
                q = mp.pi                                               # annex_f has taken x > 0, +0 and +inf
            else:
                q = mp.pi / 2                                           # x = +-0, y a number
            return s * q
        return mp.atan2(mp.mpf(y), mp.mpf(x))
    if op == "HYPOT":
        x, y = mp.mpf(a), mp.mpf(b)
        return mp.sqrt(x * x + y * y)
    x = mp.mpf(a)
    if op in ("EXP", "EXP2", "EXPM1", "SINH", "COSH") and abs(a) > 12000.0:
        if op in ("EXP", "EXP2"):
            return huge if a > 0 else tiny
        if op == "EXPM1":
            return huge if a > 0 else -1 + tiny
        return -huge if (op == "SINH" and a < 0) else huge
    if op == "TANH" and abs(a) > 100.0:
        return (1 - tiny) * (1 if a > 0 else -1)
    if op == "ATAN" and math.isinf(a):
        return mp.pi / 2 * (1 if a > 0 else -1)
    if op == "CBRT":
        return mp.cbrt(abs(x)) * (1 if a > 0 else -1)                   # the real root of a negative number
    if op == "EXP2":
        return mp.power(2, x)
    if op == "LOG2":
        return mp.log(x) / mp.log(2)
    return {"EXP": mp.exp, "EXPM1": mp.expm1, "LOG": mp.log, "LOG10": mp.log10, "LOG1P": mp.log1p, "SIN": mp.sin, "COS": mp.cos,
            "TAN": mp.tan, "ASIN": mp.asin, "ACOS": mp.acos, "ATAN": mp.atan, "SINH": mp.sinh, "COSH": mp.cosh,
            "TANH": mp.tanh}[op](x)


def _to_ld(r):
    """an mpf rounded to the 64-bit mantissa of a long double (its exponent range holds 2^+-16000)"""
    sign, man, exp, bc = r._mpf_
    if man == 0:
        return LD(0.0)
    if bc > 64:
        exp += bc - 64
        man >>= bc - 64
    v = np.ldexp(LD(man >> 32) * LD(2.0 ** 32) + LD(man & 0xffffffff), int(max(min(exp, 16300), -16400)))
    return -v if sign else v


_SCALAR_MEMO = {}


def reference(op, a, b=None):
    """-> (special [n] bool, exact [n] fp64: the Annex F result where special, ref [n] long double: the mpmath result elsewhere)
    of operand arrays of any shape, raveled.  Each distinct argument is evaluated once per process."""
    a = np.ravel(np.asarray(a, dtype=np.float64))
    bits = a.view(np.int64)[:, None]
    if b is not None:
        b = np.ravel(np.asarray(b, dtype=np.float64))
        bits = np.concatenate([bits, b.view(np.int64)[:, None]], axis=1)
    uniq, inv = np.unique(bits, axis=0, return_inverse=True)
    inv = np.ravel(inv)
    memo = _SCALAR_MEMO.setdefault(op, {})
    special, exact, ref = np.zeros(len(uniq), dtype=bool), np.zeros(len(uniq)), np.zeros(len(uniq), dtype=LD)
    with mpmath.workdps(MP_DIGITS):
        for k, key in enumerate(map(tuple, uniq.tolist())):
            got = memo.get(key)
            if got is None:
                args = [float(np.int64(v).view(np.float64)) for v in key]
                e = annex_f(op, *args)
                got = memo[key] = (True, e, LD(0.0)) if e is not None else (False, 0.0, _to_ld(mp_value(op, *args)))
            special[k], exact[k], ref[k] = got
    return special[inv], exact[inv], ref[inv]


TWO_1024 = np.ldexp(LD(1.0), 1024)


def ulps(got, ref):
    """|got - ref| in ulps of the reference: the spacing of fp64 at |ref|, 2^-1074 below the smallest normal number and 2^971 from
    2^1023 on.  An infinite result counts as 2^1024 of its sign, the value it rounds, and is exact where |ref| >= 2^1024: a
    reference at or above 2^1024 (1 - 2^-54) thus expects inf within half an ulp, and one within the tolerance of DBL_MAX accepts
    DBL_MAX or inf.  A NaN is an infinite error."""
    got = np.asarray(got, dtype=np.float64)
    g = got.astype(LD)
    g = np.where(np.isinf(got), np.sign(got).astype(LD) * TWO_1024, g)
    _, e = np.frexp(np.abs(ref))
    e = np.where(ref == 0, -2000, e)
    spacing = np.ldexp(LD(1.0), np.clip(e - 53, -1074, 971).astype(np.int32))
    with np.errstate(all="ignore"):
        err = (np.abs(g - ref) / spacing).astype(np.float64)           # an error beyond the range of fp64 is inf
    beyond = (np.abs(ref) >= TWO_1024) & np.isinf(got) & (np.sign(got) == np.sign(ref))
    return np.where(np.isnan(got), np.inf, np.where(beyond, 0.0, err))


def judge(op, got, a, b=None):
    """The verdict on the results `got` of a libm-backed opcode at the operands a, b (same shapes).
    -> (bad [n] bool: a special result that differs from the table, err [n]: ulps of the others (0 at the special ones)).
    Every argument gets one of the two verdicts."""
    got = np.ravel(np.asarray(got, dtype=np.float64))
    special, exact, ref = reference(op, a, b)
    assert got.shape == special.shape
    verdict = np.zeros(got.size, dtype=np.int8)
    bad = special & ~same_bits(got, exact)
    verdict[special] = 1
    err = np.where(special, 0.0, ulps(got, ref))
    verdict[~special] = 2
    assert (verdict > 0).all(), (op, "arguments without a verdict", int((verdict == 0).sum()))
    return bad, err


def worst(op, err, a, b=None):
    """(largest error, its argument) for the report"""
    k = int(np.argmax(err))
    a = np.ravel(a)
    return float(err[k]), (float(a[k]),) if b is None else (float(a[k]), float(np.ravel(b)[k]))


def check_selecting(program, block, got):
    """a selecting program: the kept samples, in order, bit for bit those of run_reference (the shape carries n_selected)"""
    want, keep = lowering.run_reference(program.plan_host(), program.stored(block), has_coarse=block.shape[2] == 2)
    assert got.shape == want.shape, (program.name, got.shape, want.shape, int(keep.sum()))
    same = same_bits(got, want)
    assert same.all(), (program.name, np.argwhere(~same)[:4].tolist())
    return int(keep.sum())


def check_program(program, block, got, tol=None, errors=None):
    """Compare the result rows `got` [n_out, n, s] of a non-selecting program on the stored block [3, n, s] with the references:
    run_reference bit for bit for the exact opcodes, the restated definitions for min / max, Annex F and mpmath within `tol`
    (None: the opcode's tolerance) for the libm-backed ones.  errors: dict that collects (largest ulps, argument) per opcode."""
    want, keep = lowering.run_reference(program.plan_host(), program.stored(block), has_coarse=block.shape[2] == 2)
    assert keep.all() and got.shape == want.shape, (program.name, got.shape, want.shape)
    for k, (op, sa, sb) in enumerate(program.outputs):
        a, b = program.operand(sa, block), program.operand(sb, block)
        kind = "exact" if op == "EXACT" else CASES[op][1]
        if kind == "exact":
            same = same_bits(got[k], want[k])
            assert same.all(), (program.name, k, op, _first(same, got[k], want[k], a, b))
        elif kind == "minmax":
            exp = minmax_expected(op, a, b)
            same = same_bits(got[k], exp, either_zero=(a == 0) & (b == 0) if op in ("FMAX", "FMIN") else None)
            assert same.all(), (program.name, k, op, _first(same, got[k], exp, a, b))
        else:
            bad, err = judge(op, got[k], a, b)
            table = reference(op, a, b)[1].reshape(a.shape)
            assert not bad.any(), (program.name, k, op, "special result", _first(~bad.reshape(a.shape), got[k], table, a, b))
            e, arg = worst(op, err, a, b)
            if errors is not None and e >= errors.get(op, (-1.0, None))[0]:
                errors[op] = (e, arg)
            limit = tolerance(op) if tol is None else tol
            assert e <= limit, (program.name, k, op, "ulps", e, "at", arg, "tolerance", limit)


def _first(same, got, want, a, b):
    idx = np.argwhere(~same)[:4]
    return [(tuple(int(v) for v in i), float(got[tuple(i)]), float(want[tuple(i)]), float(a[tuple(i)]) if a is not None else None,
             float(b[tuple(i)]) if b is not None else None) for i in idx]


class _HostPlan:

    def __init__(self, program):
        self.prog, self.in_rows, self.n_out = program.prog, program.in_rows, program.n_out
