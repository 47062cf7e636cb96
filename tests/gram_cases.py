"""The case tables of the extended-precision checks of the component covariance (xcov.hip) and of the bootstrap contraction
(bootstrap.hip), shared by tests/test_gram_exact_cpu.py (the reference's self-checks and the calibration of the fp64 twins) and
tests/test_gpu_gram_exact.py (the device).  Seeded NumPy data with hand-placed samples written over it: nothing here touches the
device or the package.  The reference is tests/gram_exact.py."""
import numpy as np

from tests import accum_exact as ax
from tests import gram_exact as gx
from tests.accum_cases import _inv, legendre_band

# ===========================================================================================================================
# component covariance
# ===========================================================================================================================
# T = 1 | 2 | 4 bands (M <= 16 | 32 | more); one block (M <= 64: the NaN decision in LDS) against the mask pre-pass; 129: three
# blocks (a non-adjacent off-diagonal pair); 200: a ragged last block of 8
XCOV_M = (1, 2, 16, 17, 32, 33, 64, 65, 129, 200)
RAGGED = (1, 2, 3, 17)                    # the first cuts of a level pushed in ragged chunks, then n // 3, n // 2 + 7, n - 1


def xcov_T(M):
    return 1 if M <= 16 else (2 if M <= 32 else 4)


def xcov_batch(M):
    """samples per batch of k_xcov_accum"""
    return 128 // xcov_T(M)


def xcov_big(M):
    """a size at which every sample slice makes several grid-stride trips and the last batch is ragged"""
    return 4099 if M <= 33 else (1003 if M <= 65 else 515)


def xcov_level_sizes(M):
    B = xcov_batch(M)
    return [1, B - 1, B, B + 1, 4 * B + 3, xcov_big(M)]


def dyadic_shift(M):
    """a non-trivial shift of multiples of 1 / 8: shift + 1 and shift + 0 are exact, so hand-placed f~, c~ are what they say"""
    return ((np.arange(M) * 5) % 17 - 8) / 8.0


def ragged_cuts(n):
    return sorted({0, n} | {int(x) for x in RAGGED + (n // 3, n // 2 + 7, n - 1) if 0 < x < n})


class XCase:
    """name; M; levels [(fine [M, n], coarse [M, n] | None)]; shift [M] | None.  The tolerance class of a level is
    xcov_class(M, coarse is not None)."""

    def __init__(self, name, M, levels, shift):
        self.name, self.M, self.levels, self.shift = name, M, levels, shift
        self.L = len(levels)

    def __repr__(self):
        return self.name


def xcov_class(M, paired):
    return "{}_T{}".format("pair" if paired else "level0", xcov_T(M))


def zero_component(M):
    """the component whose every value equals its shift (row and column of scale 0), None for M < 3"""
    return M // 3 if M >= 3 else None


def later_component(M):
    """a component outside the first 64-wide block (M > 64)"""
    return 64 + (M - 65) // 2


def _xcov_data(M, sizes, seed, shift):
    """components of different size and correlation around the shift; level 0 has fine values only"""
    rng = np.random.default_rng(seed)
    mix = rng.normal(size=(M, M)) / np.sqrt(M)
    a = np.zeros(M) if shift is None else shift
    out = []
    for l, n in enumerate(sizes):
        f = mix @ rng.normal(size=(M, n)) + np.linspace(-1.0, 2.0, M)[:, None] + 0.3 * rng.normal(size=(M, n)) + a[:, None]
        c = None if l == 0 else f + 0.2 * (mix @ rng.normal(size=(M, n)))
        out.append((np.ascontiguousarray(f), c))
    return out


def place_xcov(levels, M, shift):
    """Write the hand-placed samples over every level.
      every sample    component zero_component(M) equals its shift (shift None: +0.0 and -0.0 alternate)
      n == 1, pair    fine == coarse in every component: s and sp are exactly 0
      n >= 8          sample 2: fine == coarse in every component; samples 3, 4: (f~_0, c~_0, f~_j, c~_j) = (1, 0, 0, 1) and its
                      mirror with j = M - 1
      NaN, n >= 8     sample 0 (fine, component 0), sample n - 1 (coarse, component M - 1), samples B - 1 (fine, component
                      M - 1) and B (coarse, component 0) of the first batch edge where the level has them, and for M > 64 sample 5
                      in later_component(M), a component of a later block (fine).  Level 0 has no coarse values: its NaNs are all fine."""
    a = np.zeros(M) if shift is None else shift
    z, B = zero_component(M), xcov_batch(M)
    for f, c in levels:
        n = f.shape[1]
        if n == 1 and c is not None:
            c[:, 0] = f[:, 0]
        if n >= 8:
            if c is not None:
                c[:, 2] = f[:, 2]
                if M >= 2:
                    j = M - 1
                    f[0, 3], c[0, 3], f[j, 3], c[j, 3] = a[0] + 1.0, a[0], a[j], a[j] + 1.0
                    f[0, 4], c[0, 4], f[j, 4], c[j, 4] = a[0], a[0] + 1.0, a[j] + 1.0, a[j]
            lo = f if c is None else c
            f[0, 0] = np.nan
            lo[M - 1, n - 1] = np.nan
            if B - 1 < n - 1:
                f[M - 1, B - 1] = np.nan
            if B < n - 1:
                lo[0, B] = np.nan
            if M > 64:
                f[later_component(M), 5] = np.nan
        if z is not None:
            for side in (f,) if c is None else (f, c):
                keepnan = np.isnan(side[z])
                side[z] = a[z] if shift is not None else np.where(np.arange(n) % 2 == 0, 0.0, -0.0)
                side[z, keepnan] = np.nan
    return levels


_XCASES = None


def xcov_cases():
    """name -> XCase, in table order"""
    global _XCASES
    if _XCASES is not None:
        return _XCASES
    out = {}

    def add(name, M, levels, shift):
        out[name] = XCase(name, M, levels, shift)

    for M in XCOV_M:
        sizes = xcov_level_sizes(M)
        shift = dyadic_shift(M)
        # level 0 on the large size, a pair level of every size, the one-sample pair level last
        main = [sizes[-1], sizes[-1]] + sizes[1:-1] + [1]
        add("m{}".format(M), M, place_xcov(_xcov_data(M, main, 7000 + M, shift), M, shift), shift)
        # level 0 on every other size, without a shift
        for n in sizes[:-1]:
            add("m{}_level0_{}".format(M, n), M, place_xcov(_xcov_data(M, [n], 8000 + 13 * M + n, None), M, None), None)
    # M = 1024 once: 136 block pairs
    shift = dyadic_shift(1024)
    add("m1024", 1024, place_xcov(_xcov_data(1024, [40, 3], 9024, shift), 1024, shift), shift)
    # components scaled from 1e-6 to 1e6 in one matrix
    lv = _xcov_data(17, [300, 131], 9100, None)
    sc = np.logspace(-6, 6, 17)[:, None]
    add("scales_17", 17, place_xcov([(f * sc, None if c is None else c * sc) for f, c in lv], 17, None), None)
    # 1e6 + 1e-3 z with the shift 1e6
    rng = np.random.default_rng(9200)
    lv = []
    for l, n in enumerate((200, 67)):
        f = 1e6 + 1e-3 * rng.normal(size=(33, n))
        lv.append((f, None if l == 0 else f + 1e-4 * rng.normal(size=(33, n))))
    add("offset_33", 33, lv, np.full(33, 1e6))
    # a level whose every sample is dropped (a NaN somewhere in each), in LDS and through the mask pre-pass
    for M in (5, 70):
        shift = dyadic_shift(M)
        lv = place_xcov(_xcov_data(M, [50, 40, 33], 9300 + M, shift), M, shift)
        f, c = lv[1]
        for k in range(40):
            (f if k % 2 else c)[(3 * k) % M, k] = np.nan
        add("alldrop_{}".format(M), M, lv, shift)
    _XCASES = out
    return out


_XREF = {}


def xcov_reference(case):
    """the long-double sums of a case, computed once"""
    if case.name not in _XREF:
        _XREF[case.name] = gx.xcov_sums(case.levels, case.shift)
    return _XREF[case.name]


# Worst error of the fp64 twins (A: the definition; B: the identities) against the long-double reference, in units of
# 2^-53 * scale, over every level of the class in every case.  Measured and asserted by
# tests/test_gram_exact_cpu.py::test_xcov_twin_calibration_table.
XCOV_TWIN_UNITS = {
    "level0_T1": dict(s=(33.9, 33.9), sp=(49.6, 51.0)),
    "level0_T2": dict(s=(34.8, 34.8), sp=(36.2, 36.2)),
    "level0_T4": dict(s=(33.6, 33.6), sp=(28.6, 28.6)),
    "pair_T1": dict(s=(0.283, 0.211), sp=(0.144, 0.0942)),
    "pair_T2": dict(s=(5.1, 4.39), sp=(1.88, 2.95)),
    "pair_T4": dict(s=(1.22, 1.27), sp=(0.982, 1.13)),
}


def xcov_tolerance(cls, quantity):
    """max(16, 4 x the worse twin) units: the rule of tests/accum_cases.tolerance"""
    a, b = XCOV_TWIN_UNITS[cls][quantity]
    return max(16.0, 4.0 * max(a, b))


# ===========================================================================================================================
# bootstrap
# ===========================================================================================================================
DOM = (-4.0, 4.0)
MONO_DOM = (-4.0, 4.5)
LOG_DOM = (0.05, 30.0)
COMPONENT_DOMS = ((-4.0, 4.0), (-3.0, 3.5), (-5.0, 4.25), (-4.5, 3.75))
# sample positions where the kernels cut a chunk: 64-sample batches, 512-sample slices, 4096-position tiles, 32768-sample ranges
EDGES = (0, 63, 64, 511, 512, 4095, 4096, 32767, 32768)
CHECKED = (0, 15, 16, 63, 64, 256)        # and B - 1: MFMA rows of 16, 64-replicate tiles, the second group of 256


class BCase:
    """name; layout "shared" (BootstrapAccumulator: one Desc, the keep ANDed over the components) | "component"
    (ComponentBootstrapAccumulator: descs[m] and its own keep per component); descs; M; B; calls [(level, fine [M, n], coarse |
    None, sizes [B], stream)] in accum order, level 0 without coarse values, level 2 the one sample of _end_pair; seed; cls: the
    tolerance class"""

    def __init__(self, name, layout, descs, M, B, calls, seed, cls):
        self.name, self.layout, self.descs, self.M, self.B, self.calls, self.seed, self.cls = name, layout, descs, M, B, calls, seed, cls
        self.L = 3
        self.K = descs[0].size
        self.checked = sorted({b for b in CHECKED + (B - 1,) if b < B})

    def __repr__(self):
        return self.name


def _sizes(rng, n, B):
    """picks of every replicate: between n / 2 and n (a replicate of a handful of picks can sit on the zeros of a high
    polynomial, where no condition scale describes an fp64 evaluation); replicate 15 picks nothing, the last one n"""
    s = rng.integers(n // 2, n + 1, size=B)
    s[-1] = n
    if B > 15:
        s[15] = 0
    return s.astype(np.int64)


def _boot_chunk(rng, descs, M, n, paired, log, flavour):
    """seeded values inside the domains with dropped samples written over them: at the EDGES and at n - 1 a NaN or a value
    outside the domain, in the fine or the coarse row of changing components, and a NaN in every 37th sample"""
    f = 0.9 * rng.normal(size=(M, n)) + 0.1 * (np.arange(M) % 7)[:, None]
    c = f + 0.15 * rng.normal(size=(M, n)) if paired else None
    if log:
        f = np.exp(0.9 * f)
        c = None if c is None else np.exp(0.9 * c)
    if n >= 8:
        for i, pos in enumerate(sorted({p for p in EDGES + (n - 1,) if p < n})):
            m = i % M
            side = f if (c is None or i % 2 == 0) else c
            side[m, pos] = np.nan if i % 4 < 2 else descs[m].domain[1] * 1.5
        f[(np.arange(5, n, 37) // 37) % M, np.arange(5, n, 37)] = np.nan
    if flavour == "alldrop":
        f[1 % M, :] = np.nan              # shared: every sample dropped; component: component 1 % M keeps nothing
    return np.ascontiguousarray(f), c


def _end_pair(descs, M):
    """The one-sample pair chunk that is all of level 2, as the one-sample level of tests/accum_cases.py: Legendre at both ends
    of the domain (t = -1 against t = 1: every |P_k| = 1, no row's scale collapses, and the rounding of precomputed recurrence
    coefficients adds up over the degrees instead of averaging out over samples), Monomial at the upper against the lower end
    (t = 1 against 0).  Fourier (sin(k t) ~ 1e-14 at the ends, with an error of k t 2^-53 in any evaluation) and log (the keep
    decision at an end hinges on the last bit of the logarithm) take the two ordinary values of accum_cases.edge_pairs."""
    f, c = np.empty((M, 1)), np.empty((M, 1))
    for m, d in enumerate(descs):
        w = d.ref_domain[1] - d.ref_domain[0]
        if d.kind == ax.FOURIER or d.log:
            f[m, 0], c[m, 0] = _inv(d, d.ref_domain[0] + 0.6180339887498949 * w), _inv(d, d.ref_domain[0] + 0.41421356237309515 * w)
        elif d.kind == ax.MONOMIAL:
            f[m, 0], c[m, 0] = d.domain[1], d.domain[0]
        else:
            f[m, 0], c[m, 0] = d.domain
    return f, c


_BTABLE = (
    # name, layout, kind, R | K, M, log, B, ((level, n, flavour), ...)
    ("s1", "shared", ax.LEGENDRE, 1, 1, False, 1, ((0, 513, ""), (1, 65, ""), (1, 1, ""))),
    ("s16", "shared", ax.LEGENDRE, 16, 1, False, 17, ((0, 32769, ""), (1, 4097, ""))),
    ("s17", "shared", ax.FOURIER, 17, 1, False, 70, ((0, 40000, ""), (1, 511, ""))),
    ("s32", "shared", ax.LEGENDRE, 8, 4, False, 257, ((0, 4096, ""), (1, 512, ""), (1, 63, ""))),
    ("s33", "shared", ax.MONOMIAL, 11, 3, False, 70, ((0, 4095, ""), (1, 64, ""), (0, 1, ""))),
    ("s35", "shared", ax.LEGENDRE, 7, 5, False, 17, ((0, 9001, ""), (1, 513, "alldrop"), (1, 65, ""))),
    ("s64", "shared", ax.LEGENDRE, 64, 1, False, 70, ((0, 511, ""), (1, 4097, ""))),
    ("s65", "shared", ax.FOURIER, 13, 5, False, 17, ((0, 512, ""), (1, 63, ""))),
    ("s130", "shared", ax.LEGENDRE, 65, 2, False, 257, ((0, 4097, ""), (1, 513, ""))),
    ("slog", "shared", ax.LEGENDRE, 6, 2, True, 17, ((0, 4095, ""), (1, 65, ""))),
    ("c7_1", "component", ax.LEGENDRE, 7, 1, False, 17, ((0, 32769, ""), (1, 64, ""))),
    ("c7_5", "component", ax.FOURIER, 7, 5, False, 70, ((0, 40000, ""), (1, 4096, ""))),
    ("c15_5", "component", ax.MONOMIAL, 15, 5, False, 17, ((0, 513, ""), (1, 4095, ""), (1, 1, ""))),
    ("c16_5", "component", ax.LEGENDRE, 16, 5, False, 257, ((0, 4097, ""), (1, 511, ""))),
    ("c60_1", "component", ax.LEGENDRE, 60, 1, False, 70, ((0, 512, ""), (1, 9001, ""))),
    ("c15_40", "component", ax.LEGENDRE, 15, 40, False, 17, ((0, 65, ""), (1, 63, "alldrop"), (1, 513, ""))),
    ("c60_40", "component", ax.LEGENDRE, 60, 40, False, 1, ((0, 511, ""), (1, 65, ""))),     # 2440 columns: two component groups
    ("clog", "component", ax.LEGENDRE, 7, 5, True, 17, ((0, 513, ""), (1, 64, ""))),
)

_BCASES = None


def boot_cases():
    """name -> BCase, in table order"""
    global _BCASES
    if _BCASES is not None:
        return _BCASES
    out = {}
    for i, (name, layout, kind, R, M, log, B, calls) in enumerate(_BTABLE):
        rng = np.random.default_rng(4000 + i)
        base = LOG_DOM if log else (MONO_DOM if kind == ax.MONOMIAL else DOM)
        if layout == "component":
            doms = [(LOG_DOM[0] * (1 + 0.25 * (m % 3)), LOG_DOM[1]) if log else COMPONENT_DOMS[m % 4] for m in range(M)]
            descs = [ax.Desc(kind, R, d, log=log) for d in doms]
        else:
            descs = [ax.Desc(kind, R, base, log=log)] * M
        cls = "log" if log else (legendre_band(R) if kind == ax.LEGENDRE else kind)
        made, chunk_no = [], {}
        for level, n, flavour in calls:
            f, c = _boot_chunk(rng, descs, M, n, level > 0, log, flavour)
            k = chunk_no.get(level, 0)
            chunk_no[level] = k + 1
            made.append((level, f, c, _sizes(rng, n, B), (level << 20) | k))
        made.append((2,) + _end_pair(descs, M) + (_sizes(rng, 1, B), 2 << 20))
        out[name] = BCase(name, layout, descs, M, B, made, 100 + i, cls)
    _BCASES = out
    return out


def boot_rows(case, call, dtype=ax.LD, variant="A"):
    """what weighted_sums needs of one accum call: shared -> [kept_rows of the whole chunk]; component -> one per component"""
    _, f, c, _, _ = call
    if case.layout == "shared":
        return [gx.kept_rows(case.descs[0], f, c, dtype, variant)]
    return [gx.kept_rows(case.descs[m], f[m:m + 1], None if c is None else c[m:m + 1], dtype, variant) for m in range(case.M)]


def boot_keeps(case, call):
    """keep [1 | M, n] of one accum call (the fp64 decision only)"""
    _, f, c, _, _ = call
    rows = [range(case.M)] if case.layout == "shared" else [[m] for m in range(case.M)]
    out = []
    for ms in rows:
        keep = np.ones(f.shape[1], dtype=bool)
        for m in ms:
            keep &= ax.transform(case.descs[m], f[m], np.float64)[1]
            if c is not None:
                keep &= ax.transform(case.descs[m], c[m], np.float64)[1]
        out.append(keep)
    return np.stack(out)


def boot_sums(case, weights, dtype=ax.LD, variant="A", rows=None):
    """weights: per accum call the integer weights [nb, n] of nb replicates -> n [nb, L, G] and s, sp, S, SP [nb, L, G, C] with
    (G, C) = (1, M * R) for the shared layout and (M, K) for the per-component one; the calls of a level add.
    rows: per call boot_rows(case, call, dtype, variant), when the caller keeps them."""
    nb = np.atleast_2d(weights[0]).shape[0]
    G, C = (1, case.M * case.K) if case.layout == "shared" else (case.M, case.K)
    n = np.zeros((nb, case.L, G), dtype=np.int64)
    s, sp, S, SP = (np.zeros((nb, case.L, G, C), dtype=dtype) for _ in range(4))
    for i, call in enumerate(case.calls):
        level, f, c = call[0], call[1], call[2]
        per = boot_rows(case, call, dtype, variant) if rows is None else rows[i]
        for g, r in enumerate(per):
            fg, cg = (f, c) if case.layout == "shared" else (f[g:g + 1], None if c is None else c[g:g + 1])
            got = gx.weighted_sums(case.descs[g], fg, cg, weights[i], dtype, variant, rows=r)
            n[:, level, g] += got[0]
            for dst, src in zip((s, sp, S, SP), got[1:]):
                dst[:, level, g] += src
    return n, s, sp, S, SP


# Worst error of the fp64 twins of tests/accum_exact.py (A: the reference's operation order; B: the textbook recurrences;
# None where the family has one twin), weighted with rng.multinomial weights of the law of the device's, against the
# long-double reference in units of 2^-53 * scale, over every case of the class (the classes of accum_cases.TWIN_UNITS) and
# its checked replicates.  Measured and asserted by tests/test_gram_exact_cpu.py::test_boot_twin_calibration_table.
BOOT_TWIN_UNITS = {
    "legendre<=16": dict(s=(1.85, 2.0), sp=(2.04, 1.33)),
    "legendre<=64": dict(s=(1.96, 63.0), sp=(1.84, 42.0)),
    "legendre<=128": dict(s=(1.14, 63.0), sp=(0.878, 42.0)),
    "monomial": dict(s=(2.49, None), sp=(1.76, None)),
    "fourier": dict(s=(10.8, 7.32), sp=(7.41, 4.76)),
    "log": dict(s=(0.837, 0.693), sp=(0.787, 0.66)),
}


def boot_tolerance(cls, quantity):
    a, b = BOOT_TWIN_UNITS[cls][quantity]
    return max(16.0, 4.0 * max(a, b or 0.0))


def multinomial_weights(case, seed=0):
    """per accum call the weights [len(checked), n] of the checked replicates under NumPy's own multinomial: the law of the
    device's weights, not its draws (calibration only)"""
    rng = np.random.default_rng(50000 + seed + case.seed)
    out = []
    for _, f, _, sizes, _ in case.calls:
        n = f.shape[1]
        out.append(np.stack([rng.multinomial(int(sizes[b]), np.full(n, 1.0 / n)) for b in case.checked]).astype(np.int64))
    return out
