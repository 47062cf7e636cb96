"""GPU tests of the component-covariance bootstrap through the C ABI (mlmc_bootstrap_create_xcov / _set_shift / _finalize_xcov with
mlmc_bootstrap_accum / _reset / _destroy): the device sums against the long-double reference of tests/xcov_boot_cases.py built from
the weights mlmc_bootstrap_weights exports.  Counts are exact; s1 and s2 stay within max(16, 4 x the worse fp64 twin) units of
2^-53 x scale (xcov_boot_cases.tolerance, calibrated without a device by tests/test_xcov_boot_cpu.py); a zero scale demands an exact
zero.  Shapes at every edge of the kernel (xcov_boot_cases.device_shapes), both the level-0 and the pair form, a zero and a
non-zero shift.  Every test prints its worst units (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

from tests import xcov_boot_cases as xc

pytestmark = pytest.mark.gpu

SEED = 90210


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _sizes(n, B, seed):
    """picks per replicate: n, 0 and 1 first (B allowing), then uniform in 0 .. n"""
    rng = np.random.default_rng([seed, n, B])
    return np.concatenate(([n, 0, 1], rng.integers(0, n + 1, size=B)))[:B].astype(np.int64)


class Handle:
    """a mlmc_bootstrap handle of mlmc_bootstrap_create_xcov, driven through the C ABI"""

    def __init__(self, hip, M, L, B):
        self.hip, self.lib, self.M, self.L, self.B = hip, hip.lib(), M, L, B
        self.h = C.c_void_p()
        hip.check(self.lib.mlmc_bootstrap_create_xcov(M, L, B, C.byref(self.h)))
        self.alive = []

    def set_shift(self, shift, reset=True):
        shift = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
        self.hip.check(self.lib.mlmc_bootstrap_set_shift(self.h, self.hip.ptr(shift)))
        if reset:
            self.reset()

    def reset(self):
        self.hip.check(self.lib.mlmc_bootstrap_reset(self.h))

    def accum(self, level, f, c, sizes, stream, seed=SEED):
        self.alive.append((f, c))
        sizes = np.ascontiguousarray(sizes, dtype=np.int64)
        self.hip.check(self.lib.mlmc_bootstrap_accum(self.h, level, self.hip.ptr(f), self.hip.ptr(c), int(f.shape[1]), self.hip.ptr(sizes),
                                                     seed, stream))

    def finalize(self):
        M, L, B = self.M, self.L, self.B
        n = np.full((B, L), -1, dtype=np.int64)
        s1 = np.full((B, L, M), np.nan)
        s2 = np.full((B, L, M, M), np.nan)
        self.hip.check(self.lib.mlmc_bootstrap_finalize_xcov(self.h, self.hip.ptr(n), self.hip.ptr(s1), self.hip.ptr(s2)))
        self.alive = []
        return n, s1, s2

    def close(self):
        if self.h is not None:
            self.lib.mlmc_bootstrap_destroy(self.h)
            self.h = None


def _weights(n, sizes, stream, seed=SEED):
    from mlmc_amd import engine
    w = engine.bootstrap_weights(n, sizes, seed, stream)
    assert np.array_equal(w.sum(axis=1), sizes) and w.min() >= 0
    return w.astype(np.int64)


def _compare(tag, got, ref, cls):
    """counts exactly, s1 / s2 within the tolerance of the class; -> (units of s1, units of s2)"""
    n, s1, s2 = got
    r_n, r_s1, r_s2, U1, U2 = ref
    assert np.array_equal(n, r_n), (tag, n, r_n)
    assert np.array_equal(s2, np.swapaxes(s2, -1, -2)), tag                      # bitwise symmetric
    u1, u2 = xc.units(s1, r_s1, U1), xc.units(s2, r_s2, U2)
    print("{:34s} {:6s} worst units s1 {:8.3g} (tol {:g})  s2 {:8.3g} (tol {:g})".format(tag, cls, u1, xc.tolerance(cls, "s1"), u2,
                                                                                       xc.tolerance(cls, "s2")))
    assert u1 <= xc.tolerance(cls, "s1"), (tag, cls, u1)
    assert u2 <= xc.tolerance(cls, "s2"), (tag, cls, u2)
    return u1, u2


def _run_shape(hip, M, n, B, offset=0.0):
    """level 0 (no coarse values) and level 1 (a pair) of one handle, with a zero and a non-zero shift"""
    f0, _ = xc.make_chunk(M, n, 1, False, offset)
    f1, c1 = xc.make_chunk(M, n, 2, True, offset)
    sizes = [_sizes(n, B, 1), _sizes(n, B, 2)]
    w = [_weights(n, sizes[0], 17), _weights(n, sizes[1], (1 << 20) | 3)]
    d0, d1, dc1 = _dev(f0), _dev(f1), _dev(c1)
    h = Handle(hip, M, 2, B)
    try:
        for kind in ("zero", "mean"):
            shift = xc.make_shift(M, kind, offset)
            h.reset()                                                            # (a shift cannot be set while chunks are pending)
            h.set_shift(shift)
            h.accum(0, d0, None, sizes[0], 17)
            h.accum(1, d1, dc1, sizes[1], (1 << 20) | 3)
            n_d, s1, s2 = h.finalize()
            for level, cls, f, c in ((0, "level0", f0, None), (1, "pair", f1, c1)):
                ref = xc.weighted_sums(f, c, shift, w[level])
                _compare("M{} n{} B{} shift {}".format(M, n, B, kind), (n_d[:, level], s1[:, level], s2[:, level]), ref, cls)
                zero = np.flatnonzero(sizes[level] == 0)                         # sizes[b] = 0 gives zeros
                assert np.all(n_d[zero, level] == 0) and np.all(s1[zero, level] == 0.0) and np.all(s2[zero, level] == 0.0)
    finally:
        h.close()


@pytest.mark.parametrize("M,n,B", xc.device_shapes(), ids=lambda v: str(v))
def test_device_sums_against_the_long_double_reference(hip, M, n, B):
    _run_shape(hip, M, n, B)


def test_large_offset_with_and_without_the_shift(hip):
    """|mean| = 100 std: the 'mean' shift removes the cancellation of the raw second moments, the zero shift keeps it -- both stay
    within the tolerance of their own scale"""
    _run_shape(hip, 5, 4097, 3, offset=100.0)


def test_a_nan_in_one_component_drops_the_sample_from_every_entry(hip):
    M, n, B = 3, 200, 5
    f, c = xc.make_chunk(M, n, 5, True, nan=False)
    f[1, 7] = np.nan                                                             # fine, one component
    c[2, 9] = np.nan                                                             # coarse, another one
    f_all, c_all = f.copy(), c.copy()
    f_all[:, [7, 9]] = np.nan                                                    # the same samples dropped in every component
    c_all[:, [7, 9]] = np.nan
    sizes = np.full(B, n, dtype=np.int64)
    w = _weights(n, sizes, 4)
    keep = np.ones(n, dtype=bool)
    keep[[7, 9]] = False
    out = []
    for ff, cc in ((f, c), (f_all, c_all)):
        h = Handle(hip, M, 1, B)
        try:
            h.set_shift([0.1, 0.2, 0.3])
            h.accum(0, _dev(ff), _dev(cc), sizes, 4)
            out.append(h.finalize())
        finally:
            h.close()
    assert np.array_equal(out[0][0][:, 0], (w * keep).sum(axis=1)) and np.any(w[:, [7, 9]] > 0)
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    _compare("nan fine / coarse", tuple(v[:, 0] for v in out[0]), xc.weighted_sums(f, c, [0.1, 0.2, 0.3], w), "pair")


def test_runs_are_bit_identical_and_a_replicate_does_not_depend_on_B(hip):
    M, n = 5, 9001
    f, c = xc.make_chunk(M, n, 8, True)
    d, dc = _dev(f), _dev(c)
    sizes = _sizes(n, 300, 3)
    shift = xc.make_shift(M, "mean")

    def run(B):
        h = Handle(hip, M, 2, B)
        try:
            h.set_shift(shift)
            h.accum(0, d, None, sizes[:B], 1)
            h.accum(1, d, dc, sizes[:B], 2)
            return h.finalize()
        finally:
            h.close()
    a, b, small = run(300), run(300), run(50)
    for x, y, z in zip(a, b, small):
        assert np.array_equal(x, y)                                              # two runs
        assert np.array_equal(x[:50], z)                                         # replicates 0 .. 49 of B = 300 equal B = 50


def test_two_chunks_of_one_level_add(hip):
    M, B = 4, 6
    parts = [xc.make_chunk(M, n, 20 + i, True) for i, n in enumerate((700, 4200))]
    sizes = [_sizes(f.shape[1], B, 30 + i) for i, (f, _) in enumerate(parts)]
    shift = xc.make_shift(M, "mean")
    h = Handle(hip, M, 2, B)
    try:
        h.set_shift(shift)
        for i, (f, c) in enumerate(parts):
            h.accum(1, _dev(f), _dev(c), sizes[i], (1 << 20) | i)
        n_d, s1, s2 = h.finalize()
    finally:
        h.close()
    assert np.all(n_d[:, 0] == 0) and np.all(s1[:, 0] == 0.0) and np.all(s2[:, 0] == 0.0)      # the untouched level
    refs = [xc.weighted_sums(f, c, shift, _weights(f.shape[1], sizes[i], (1 << 20) | i)) for i, (f, c) in enumerate(parts)]
    _compare("two chunks", (n_d[:, 1], s1[:, 1], s2[:, 1]), tuple(a + b for a, b in zip(*refs)), "pair")


def test_host_uploaded_and_device_resident_inputs_agree_bit_for_bit(hip):
    """a chunk uploaded from host arrays and the same values resident in another device allocation (views into a larger buffer,
    8 bytes off its start): the same bits"""
    import torch
    M, n, B = 6, 5000, 70
    f, c = xc.make_chunk(M, n, 31, True)
    sizes = _sizes(n, B, 9)
    big = torch.empty(2 * M * n + 1, dtype=torch.float64, device="cuda")
    rf, rc = big[1:1 + M * n].view(M, n), big[1 + M * n:].view(M, n)
    rf.copy_(_dev(f))
    rc.copy_(_dev(c))
    torch.cuda.synchronize()
    out = []
    for ff, cc in ((_dev(f), _dev(c)), (rf, rc)):
        h = Handle(hip, M, 1, B)
        try:
            h.accum(0, ff, cc, sizes, 5)
            out.append(h.finalize())
        finally:
            h.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_each_finalize_refuses_the_other_handles(hip):
    from mlmc_amd import Legendre
    lib = hip.lib()
    fn = Legendre(4, (-2.0, 2.0))
    h_x, h_s, h_m = C.c_void_p(), C.c_void_p(), C.c_void_p()
    hip.check(lib.mlmc_bootstrap_create_xcov(2, 1, 3, C.byref(h_x)))
    hip.check(lib.mlmc_bootstrap_create(fn._basis_handle(), 2, 1, 3, C.byref(h_s)))
    bases = (C.c_void_p * 2)(fn._basis_handle().value, fn._basis_handle().value)
    hip.check(lib.mlmc_bootstrap_create_multi(2, C.cast(bases, C.c_void_p), 4, 1, 3, C.byref(h_m)))
    n = np.zeros(64, dtype=np.int64)
    a, b = np.zeros(256), np.zeros(256)
    args = (hip.ptr(n), hip.ptr(a), hip.ptr(b))
    try:
        for fin, h, needle in ((lib.mlmc_bootstrap_finalize, h_x, "mlmc_bootstrap_finalize: .*mlmc_bootstrap_create_xcov"),
                               (lib.mlmc_bootstrap_finalize_multi, h_x, "mlmc_bootstrap_finalize_multi: .*mlmc_bootstrap_create_xcov"),
                               (lib.mlmc_bootstrap_finalize_xcov, h_s, "mlmc_bootstrap_finalize_xcov: .*mlmc_bootstrap_create "),
                               (lib.mlmc_bootstrap_finalize_xcov, h_m, "mlmc_bootstrap_finalize_xcov: .*mlmc_bootstrap_create_multi")):
            with pytest.raises(hip.MlmcHipError, match=needle):
                hip.check(fin(h, *args))
        with pytest.raises(hip.MlmcHipError, match="mlmc_bootstrap_set_shift: not a component-covariance handle"):
            hip.check(lib.mlmc_bootstrap_set_shift(h_s, None))
        hip.check(lib.mlmc_bootstrap_finalize_xcov(h_x, *args))                   # its own finalize serves it
    finally:
        for h in (h_x, h_s, h_m):
            lib.mlmc_bootstrap_destroy(h)


def test_set_shift_rules_and_create_limits(hip):
    lib = hip.lib()
    M, n, B = 2, 100, 3
    f, _ = xc.make_chunk(M, n, 40, False)
    h = Handle(hip, M, 1, B)
    try:
        with pytest.raises(hip.MlmcHipError, match=r"mlmc_bootstrap_set_shift: shift\[1\] is not finite"):
            h.set_shift([0.0, np.nan])
        h.set_shift([1.0, 2.0])
        h.accum(0, _dev(f), None, _sizes(n, B, 1), 0)
        with pytest.raises(hip.MlmcHipError, match="mlmc_bootstrap_set_shift: pushes are pending; reset the accumulator first"):
            h.set_shift(None, reset=False)
        first = h.finalize()
        with pytest.raises(hip.MlmcHipError, match="pushes are pending"):        # the totals stay after finalize: still pending
            h.set_shift(None, reset=False)
        h.reset()
        h.set_shift(None, reset=False)                                           # takes effect at the next reset, not before
        h.accum(0, _dev(f), None, _sizes(n, B, 1), 0)
        again = h.finalize()
        for a, b in zip(first, again):
            assert np.array_equal(a, b)
        h.reset()
        h.accum(0, _dev(f), None, _sizes(n, B, 1), 0)
        zero = h.finalize()
        assert not np.array_equal(zero[1], first[1])
        _compare("shift after reset", tuple(v[:, 0] for v in zero), xc.weighted_sums(f, None, None, _weights(n, _sizes(n, B, 1), 0)),
                 "level0")
    finally:
        h.close()
    out = C.c_void_p()
    for M_bad in (0, 1025):
        assert lib.mlmc_bootstrap_create_xcov(M_bad, 1, 4, C.byref(out)) != 0
        assert "mlmc_bootstrap_create_xcov: M = {}".format(M_bad) in lib.mlmc_last_error().decode()
    assert lib.mlmc_bootstrap_create_xcov(1024, 1, 600, C.byref(out)) != 0      # 600 x 525825 doubles = 2.35 GiB
    assert "at most 2048 MiB" in lib.mlmc_last_error().decode()
