"""The opcode cases of tests/expr_cases.py checked on the host: every opcode has a case, the cases know the library's `heavy`
list, the library would accept every program, the operand forms of one opcode agree, the argument sets hold the edges they claim
to, and the reference machinery (Annex F table, mpmath, the ulp measure) agrees with an independent source: NumPy's libm run
through lowering.run_reference on the same programs.  No GPU."""
import math
import os

import numpy as np
import pytest

from mlmc_amd.quantity import lowering
from tests import expr_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = math.nan, math.inf


@pytest.fixture(scope="module")
def programs():
    return ec.all_programs()


def _blocks(program):
    pair = ec.arguments(ec.CASES[program.op][0])
    return pair, pair[:, :, :1]


def test_every_opcode_has_a_case():
    assert set(ec.CASES) == set(lowering._OP_NAMES) and len(lowering._OP_NAMES) == 54
    assert sorted(ec.STRUCTURE + ec.BINARY + ec.UNARY + ec.COMPARE + ec.LOGIC2) == sorted(lowering._OP_NAMES)
    in_family = [op for ops in ec.FAMILIES.values() for op in ops]
    assert sorted(in_family) == sorted(lowering._OP_NAMES)                 # each opcode runs in exactly one family
    assert set(ec.OBSERVED) == set(ec.LIBM) == {op for op, (_, ref) in ec.CASES.items() if ref == "libm"}
    for op in lowering._OP_NAMES:
        built = ec.forms(op)
        assert built, op
        want = {"rr", "chain"} | ({"imm_a", "imm_b"} if op in lowering._IMM_OK else set())
        if op not in ec.HEAVY:
            want |= {"in_heavy"}
        if ec.CASES[op][0] != "structure":
            assert set(built) == want, (op, set(built))
        for program in built.values():                                     # the opcode really is in its programs
            assert any(word & lowering.OP_MASK == ec.OP[op] for word, *_ in program.prog), program.name


def test_heavy_list_matches_the_library():
    text = open(os.path.join(ROOT, "mlmc_amd", "csrc", "expr.hip")).read()
    assert ec.heavy_list_of_source(text) == set(ec.HEAVY)
    assert set(ec.HEAVY) - set(ec.LIBM) == {"MOD", "FMOD"} and len(ec.LIBM) == 20
    for op in lowering._OP_NAMES:                                          # ... and each kernel switch guards the same opcodes
        guarded = "case MLMC_X_{}: if (HEAVY)".format(op) in text
        assert guarded == (op in ec.HEAVY), op


def test_library_would_accept_every_program(programs):
    for program in programs:
        selects, heavy = ec.validate(program.prog, program.n_regs, len(program.in_rows), program.n_out)
        assert selects == program.selects, program.name
        ops = {lowering._OP_NAMES[word & lowering.OP_MASK] for word, *_ in program.prog}
        assert heavy == bool(ops & ec.HEAVY)
        if program.form == "in_heavy":
            assert heavy and program.op not in ec.HEAVY
        elif program.op in ec.HEAVY:
            assert ops & ec.HEAVY == {program.op}, program.name           # a heavy opcode runs alone
        elif ec.CASES[program.op][0] != "structure":
            assert not heavy, program.name
        # forced to 1, 2 or 4 samples per thread, the register file of a pair block stays within the 64 KB the library allows
        assert program.n_regs * 2 * 4 * 256 * 8 <= 65536, program.name
        assert len(program.in_rows) == (65 if program.table else 3)
    with pytest.raises(AssertionError):
        ec.validate([ec._i("LOAD", 0, 0), ec._i("NEG", 1, a=0, imm=1.0, flags=ec.IMM_A), ec._i("STORE", a=1)], 2, 1, 1)
    with pytest.raises(AssertionError):
        ec.validate([ec._i("LOAD", 0, 0), ec._i("ADD", 1, a=0, b=1), ec._i("STORE", a=1)], 2, 1, 1)


def test_operand_forms_agree(programs):
    """every form of an opcode gives, under run_reference, NumPy's function of the operands that `outputs` names: so the
    immediate, chained and NO_WB forms give the rows of the register-register form"""
    for program in programs:
        for block in _blocks(program):
            got, keep = lowering.run_reference(program.plan_host(), program.stored(block), has_coarse=block.shape[2] == 2)
            if program.selects:
                flag = {"none": np.zeros(block.shape[1], dtype=bool), "all": np.ones(block.shape[1], dtype=bool)}.get(
                    program.form, (block[ec.ROW_X] > 0.4).all(axis=1))
                assert np.array_equal(keep, flag), program.name
                assert program.form != "ragged" or 0.1 < keep.mean() < 0.4
            for k, (op, sa, sb) in enumerate(program.outputs):
                a, b = program.operand(sa, block), program.operand(sb, block)
                want = ec.host_apply(op, a, b)[keep]
                zeros = (a[keep] == 0) & (b[keep] == 0) if op in ec.MINMAX else None
                assert ec.same_bits(got[k], want, either_zero=zeros).all(), (program.name, k)


def test_reference_machinery_against_numpy(programs):
    """NumPy's libm through run_reference, judged like the device: the special results of the Annex F table bit for bit, below
    1 ulp of mpmath elsewhere; the exact opcodes and the restated min / max pass their own comparison"""
    errors = {}
    for program in programs:
        if program.selects:
            continue
        for block in _blocks(program):
            got, _ = lowering.run_reference(program.plan_host(), program.stored(block), has_coarse=block.shape[2] == 2)
            for k, (op, sa, sb) in enumerate(program.outputs):             # NumPy's max(+0, -0) depends on its SIMD path
                if op in ("MAXIMUM", "MINIMUM"):
                    a, b = program.operand(sa, block), program.operand(sb, block)
                    got[k] = np.where((a == 0) & (b == 0), ec.minmax_expected(op, a, b), got[k])
            ec.check_program(program, block, got, tol=ec.HOST_ULPS, errors=errors)
    assert set(errors) == set(ec.LIBM)
    print()
    for op in ec.LIBM:
        print("host {:6s} {:6.3f} ulps at {}".format(op, *errors[op]))


def test_ulps_and_overflow_rule():
    LD = ec.LD
    one = np.array([1.0])
    assert ec.ulps(np.nextafter(one, 2.0), one.astype(LD))[0] == 1.0
    assert ec.ulps(np.nextafter(one, 0.0), one.astype(LD))[0] == 0.5      # in ulps of the reference, not of the result
    assert ec.ulps(np.array([0.0]), np.array([5e-324], dtype=LD))[0] == 1.0
    assert ec.ulps(np.array([2e-308]), np.array([2e-308], dtype=LD) + LD(5e-324))[0] == 1.0
    assert ec.ulps(np.array([NAN]), one.astype(LD))[0] == INF
    top = np.array([ec.DBL_MAX], dtype=LD)
    half = np.ldexp(LD(1.0), 970)                                          # half an ulp at DBL_MAX
    threshold = top + half                                                 # 2^1024 (1 - 2^-54): the least value that rounds to inf
    assert ec.ulps(np.array([INF]), threshold)[0] == 0.5 and ec.ulps(np.array([ec.DBL_MAX]), threshold)[0] == 0.5
    assert ec.ulps(np.array([INF]), top)[0] == 1.0                         # within a tolerance >= 1 of DBL_MAX: inf passes
    assert ec.ulps(np.array([INF]), ec.TWO_1024 * LD(4.0))[0] == 0.0
    assert ec.ulps(np.array([-INF]), ec.TWO_1024 * LD(4.0))[0] > 1e3       # the wrong sign
    assert ec.ulps(np.array([ec.DBL_MAX]), ec.TWO_1024 * LD(4.0))[0] > 1e3
    assert ec.ulps(np.array([INF]), np.array([1e300], dtype=LD))[0] > 1e3


def test_annex_f_table_spot_values():
    f = ec.annex_f
    same = lambda got, want: bool(ec.same_bits(got, want)) if got is not None else False
    for op, a, b, want in (("POW", NAN, 0.0, 1.0), ("POW", NAN, -0.0, 1.0), ("POW", 1.0, NAN, 1.0), ("POW", -8.0, 1.0 / 3.0, NAN),
                           ("POW", 0.0, -3.0, INF), ("POW", -0.0, -3.0, -INF), ("POW", -0.0, -2.0, INF), ("POW", -0.0, 3.0, -0.0),
                           ("POW", -1.0, INF, 1.0), ("POW", -INF, -3.0, -0.0), ("POW", -INF, 2.0, INF), ("POW", 0.5, -INF, INF),
                           ("ATAN2", 0.0, 1.0, 0.0), ("ATAN2", -0.0, 0.0, -0.0), ("ATAN2", -3.0, INF, -0.0), ("ATAN2", NAN, 1.0, NAN),
                           ("HYPOT", INF, NAN, INF), ("HYPOT", NAN, -INF, INF), ("HYPOT", NAN, 1.0, NAN)):
        assert same(f(op, a, b), want), (op, a, b)
    for op, a, want in (("LOG", 0.0, -INF), ("LOG", -0.0, -INF), ("LOG2", -1.0, NAN), ("LOG10", 1.0, 0.0), ("LOG1P", -1.0, -INF),
                        ("LOG1P", -0.0, -0.0), ("LOG1P", -2.0, NAN), ("EXP", -INF, 0.0), ("EXPM1", -INF, -1.0), ("EXPM1", -0.0, -0.0),
                        ("SIN", -0.0, -0.0), ("SIN", INF, NAN), ("COS", -INF, NAN), ("TAN", -0.0, -0.0), ("ASIN", -0.0, -0.0),
                        ("ASIN", 1.5, NAN), ("ACOS", 1.0, 0.0), ("ACOS", -1.5, NAN), ("ATAN", -0.0, -0.0), ("SINH", -INF, -INF),
                        ("COSH", -INF, INF), ("TANH", -INF, -1.0), ("TANH", -0.0, -0.0), ("CBRT", -0.0, -0.0), ("CBRT", -INF, -INF)):
        assert same(f(op, a), want), (op, a)
    import mpmath
    with mpmath.workdps(ec.MP_DIGITS):                                     # numbers, not table entries
        assert f("ATAN2", 0.0, -1.0) is None and ec.mp_value("ATAN2", -0.0, -1.0) == -mpmath.pi
        assert ec.mp_value("ATAN2", INF, -INF) == 3 * mpmath.pi / 4 and ec.mp_value("ATAN2", -2.0, 0.0) == -mpmath.pi / 2
        assert ec.mp_value("CBRT", -27.0) == -3 and ec.mp_value("POW", -2.0, 3.0) == -8 and ec.mp_value("POW", -2.0, -2.0) == 0.25


def test_argument_sets_hold_the_named_edges():
    x = ec.arguments("unary")[ec.ROW_A, :, 0]
    assert 900 <= x.size and x.size > 4 * 256                              # a second, ragged block even at four samples per thread
    have = lambda v: bool((ec.same_bits(x, v)).any())
    for m in ec.UNARY_MAGNITUDES:
        assert have(m) and have(-m), m
        if 0.0 < m:
            assert have(np.nextafter(m, 0.0)) and (m == ec.DBL_MAX or have(np.nextafter(m, INF))), m
    assert have(NAN) and have(INF) and have(-INF) and have(-0.0) and have(5e-324) and have(2.5)
    assert np.array_equal(ec.arguments("unary")[:, :, 1], ec.arguments("unary")[:, ::-1, 0], equal_nan=True)
    blk = ec.arguments("binary")
    assert np.array_equal(blk[:, :, 1], blk[:, ::-1, 0], equal_nan=True)   # the coarse side: the same set in reversed order
    a, b = blk[ec.ROW_A, :, 0], blk[ec.ROW_B, :, 0]
    assert 55 <= ec.binary_values().size <= 65 and a.size == ec.binary_values().size ** 2

    def pair(pa, pb):
        return bool((pa(a) & pb(b)).any())

    is_ = lambda v: (lambda t: ec.same_bits(t, v))
    integer = lambda t: np.isfinite(t) & (t == np.floor(t)) & (t != 0)
    subnormal = lambda t: (t != 0) & (np.abs(t) < ec.DBL_MIN)
    neg = lambda t: np.isfinite(t) & (t < 0)
    assert pair(neg, integer) and pair(neg, lambda t: np.isfinite(t) & ~integer(t) & (t != 0))     # pow(neg, integer / not)
    assert pair(is_(NAN), is_(0.0)) and pair(is_(NAN), is_(-0.0)) and pair(is_(1.0), is_(NAN))     # pow(x, +-0), pow(1, NaN)
    assert pair(is_(0.0), neg) and pair(is_(-0.0), neg) and pair(is_(-0.0), is_(-3.0))             # pow(+-0, neg)
    for y in (0.0, -0.0, INF, -INF):                                                              # atan2: zeros and infinities
        for z in (0.0, -0.0, INF, -INF):
            assert pair(is_(y), is_(z)), (y, z)
    assert pair(is_(INF), is_(NAN)) and pair(is_(NAN), is_(-INF))                                  # hypot(inf, NaN)
    assert pair(is_(1e200), is_(1e200)) and pair(subnormal, subnormal)
    assert pair(is_(1e300), is_(3.0)) and pair(np.isfinite, subnormal)                             # fmod(1e300, 3), fmod(x, subnormal)
    assert pair(np.isfinite, neg) and pair(np.isfinite, np.isinf)                                  # remainder by negative / infinite
    for v in (1.0 / 3.0, -1.0 / 3.0, 0.5, -0.5, 1.5, -1.5, ec.DBL_MAX, 1e-300):
        assert pair(is_(v), is_(v))
    imm = np.array(ec.IMMEDIATES)
    for v in (0.0, -0.0, 1.0, 0.5, 2.0, -3.0, 1.0 / 3.0, 1e300, INF, NAN):
        assert ec.same_bits(imm, v).any(), v
    # the comparisons see pairs whose two sides disagree, so the pair rule (both sides must pass) changes the flag
    lt_f, lt_c = blk[ec.ROW_A, :, 0] < blk[ec.ROW_B, :, 0], blk[ec.ROW_A, :, 1] < blk[ec.ROW_B, :, 1]
    assert (lt_f & ~lt_c).any() and (~lt_f & lt_c).any() and (lt_f & lt_c).any()
