"""The case table of the extended-precision checks of the covariance kernels, shared by tests/test_cov_exact_cpu.py (calibration
of the fp64 twins) and tests/test_gpu_cov_exact.py (the device).  Plain NumPy data; the linearisation tables are host arithmetic
of the library (no device).  Batch and grid sizes are read out of mlmc_amd/csrc/cov.hip (kernel_constants)."""
import os
import re

import numpy as np

from tests import accum_cases as ac
from tests import accum_exact as ax
from tests import cov_exact as cx
from tests.gram_cases import ragged_cuts                  # noqa: F401  (the device module cuts its chunks with it)
from tests.util import level_arrays

DOM, MONO_DOM, LOG_DOM = ac.DOM, ac.MONO_DOM, ac.LOG_DOM
STEPS = [0.5, 0.1]
N_CU = 256                                # compute units of the MI355X: the long levels exceed a full grid of that many

LEGENDRE_R = (1, 5, 16, 17, 32, 33, 48, 49, 64, 65, 80, 100, 128, 129, 200)
FOURIER_R = (9, 33, 65)
SPLINE_R = (8, 37, 128)
MONOMIAL_R = (8, 33, 52)
LOG_R = (20, 50)
FULL_R = (1, 5, 17, 33, 64, 65, 100, 129)                  # every level size of the kernel's batch; the others a shorter list
LONG_R = {"t1": 1, "t2": 17, "t4": 33, "wide": 65}         # the smallest R of a kernel takes the level of more than a grid
MONO_REF = (0.0, 1.0)


# ---------------------------------------------------------------------------------------------------------------------------
# what the code says about its batches
# ---------------------------------------------------------------------------------------------------------------------------
_CONSTANTS = None
_COV_BATCH_BODY = "return (T <= 2 && !wide && !vals) ? (pair ? 128 : 256) : ((wide && pair && !vals) ? MLMC_COV_WIDE_BATCH : 64);"


_GRID_LINES = (
    "int blocks = rt().n_cu * ((bi != bj) ? ((pair && MLMC_COV_WIDE_BATCH < 64) ? 2 : 1) : (T == 1 ? 4 : (T == 4 ? COV_T4_WGS : 2)));",
    "int blocks = rt().n_cu * (wide ? 1 : 2);          // two term windows: 135 KB of LDS, one workgroup per CU",
)


def kernel_constants():
    """{"t4_batch", "wide_batch", "t4_wgs"} from the #defines of cov.hip; cov_batch() must read as this table assumes it"""
    global _CONSTANTS
    if _CONSTANTS is None:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mlmc_amd", "csrc", "cov.hip")
        with open(path) as fh:
            src = fh.read()
        out = {}
        for key, name in (("t4_batch", "MLMC_COV_T4_BATCH"), ("wide_batch", "MLMC_COV_WIDE_BATCH"), ("t4_wgs", "MLMC_COV_T4_WGS")):
            m = re.search(r"#define\s+" + name + r"\s+(\d+)", src)
            assert m, name
            out[key] = int(m.group(1))
        assert _COV_BATCH_BODY in src, "cov_batch() has changed: revisit batches()"
        assert "constexpr int COV_BATCH = 64;" in src, "COV_BATCH (the values route) has changed: revisit batches()"
        for line in _GRID_LINES:                      # the workgroups per CU that grid() restates
            assert line in src, "a launch factor has changed: revisit grid(): " + line
        _CONSTANTS = out
    return _CONSTANTS


def kernel_of(R, values=False):
    """the kernel a covariance of R terms selects: "t1" | "t2" (generic, T = 1, 2), "t4" (64 terms), "wide" (64 x 64 blocks of
    65..128 terms), "vals" (from values: more than 128 terms, TransformedMoments)"""
    if values or R > 128:
        return "vals"
    return "t1" if R <= 16 else "t2" if R <= 32 else "t4" if R <= 64 else "wide"


def batches(kernel):
    """(pairs per batch, samples without coarse values per batch)"""
    k = kernel_constants()
    return {"t1": (128, 256), "t2": (128, 256), "t4": (k["t4_batch"], 2 * k["t4_batch"]), "wide": (k["wide_batch"], 2 * k["t4_batch"]),
            "vals": (64, 64)}[kernel]


def grid(kernel):
    """workgroups of a full grid (pair levels): the factors of launch_cov_accum and launch_cov_from_values, whose lines
    kernel_constants() pins (_GRID_LINES)"""
    k = kernel_constants()
    return N_CU * {"t1": 4, "t2": 2, "t4": k["t4_wgs"], "wide": 2 if k["wide_batch"] < 64 else 1, "vals": 2}[kernel]


def band(kind, R, log=False, values=False):
    if log:
        return "log"
    if values:
        return "transformed" if R <= 128 else "transformed>128"
    if kind == ax.LEGENDRE:
        for top in (16, 32, 64, 128, 256, 512):
            if R <= top:
                return "legendre<={}".format(top)
        raise ValueError(R)
    return "{}{}".format(kind, R) if kind == ax.SPLINE else kind


# ---------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------
def _level(n, kind, seed, M=1, nan_every=0, fn=None):
    """kind "0": fine values only; "pair": coarse = fine + small; "indep": coarse an independent draw"""
    f, c = level_arrays([n, n], STEPS, M, nan_every, seed=seed)[1]
    if kind == "0":
        c = None
    elif kind == "indep":
        c = level_arrays([n, n], STEPS, M, 0, seed=seed + 7919)[1][0]
    f = np.ascontiguousarray(f if fn is None else fn(f))
    c = None if c is None else np.ascontiguousarray(c if fn is None else fn(c))
    return f, c


def drop_positions(n, B):
    """samples 0, B - 1, B and n - 1 of a level of 8 or more samples"""
    return [] if n < 8 else sorted({0, n - 1} | {p for p in (B - 1, B) if p < n})


def place(levels, desc, kernel):
    """accum_cases.place_edges, then a NaN or a value outside the domain at samples 0, B - 1, B, n - 1 (B: the batch of the
    level's kernel), alternately in fine only and in coarse only"""
    ac.place_edges(levels, [desc])
    lo, hi = desc.domain
    outside = [np.nan, hi + 1.0 if desc.safe_eval else np.nan, np.nan, 0.0 if desc.log else (lo - 1.0 if desc.safe_eval else np.nan)]
    for f, c in levels:
        n = f.shape[1]
        B = batches(kernel)[0 if c is not None else 1]
        for i, p in enumerate(drop_positions(n, B)):
            side = f if (c is None or i % 2 == 0) else c
            other = c if side is f else f
            side[i % side.shape[0], p] = outside[i]
            if other is not None and not np.all(np.isfinite(other[:, p])):
                other[:, p] = 0.25 * (lo + hi) if not desc.log else 1.0
    return levels


class Case:
    """name; desc; levels [(fine [M, n], coarse [M, n] | None)]; kernel; routes (names of ROUTES the device runs);
    matrix (TransformedMoments) | None; entry "cov" | "diff" (MOMENTS mode of TransformedMoments: the difference Gram)"""

    def __init__(self, name, desc, levels, kernel, routes, matrix=None, entry="cov"):
        self.name, self.desc, self.levels, self.kernel, self.routes = name, desc, levels, kernel, tuple(routes)
        self.matrix, self.entry = matrix, entry
        self.M, self.L = levels[0][0].shape[0], len(levels)
        self.Rout = desc.size if matrix is None else matrix.shape[0]
        self.band = band(desc.kind, desc.size, desc.log, matrix is not None)
        if entry == "diff":
            self.band = self.band.replace("transformed", "diffgram")

    def __repr__(self):
        return self.name


# route -> environment; "lin*": every chunk on the linearised route (threshold 0)
ROUTES = {
    "direct": {"MLMC_HIP_LINEARIZE": "0"},
    "lin": {"MLMC_HIP_LINEARIZE_MIN_N": "0"},
    "lin_cheb0": {"MLMC_HIP_LINEARIZE_MIN_N": "0", "MLMC_HIP_LINEARIZE_CHEB": "0"},
    "lin_rowsums0": {"MLMC_HIP_LINEARIZE_MIN_N": "0", "MLMC_HIP_LINEARIZE_ROWSUMS": "0"},
    "lin_level0_0": {"MLMC_HIP_LINEARIZE_MIN_N": "0", "MLMC_HIP_LINEARIZE_LEVEL0": "0"},
}
ALL_ENV = sorted({k for env in ROUTES.values() for k in env})


def lin_eligible(desc, matrix=None):
    """api.hip, mlmc_accum_create: 17..128 plain Legendre or monomial moments, clipped, reference domain inside [-1, 1]"""
    return (matrix is None and desc.kind in (ax.LEGENDRE, ax.MONOMIAL) and 16 < desc.size <= 128 and desc.safe_eval
            and max(abs(desc.ref_domain[0]), abs(desc.ref_domain[1])) <= 1.0)


def lin0(case, route):
    """the levels without coarse values of this route need no matrix pass (second moments linearised too)"""
    return route.startswith("lin") and route != "lin_level0_0" and lin_eligible(case.desc, case.matrix) and case.desc.size <= 64


def level_sizes(kernel, short=False):
    Bp, B0 = batches(kernel)
    if short:
        return [("0", B0 + 1), ("pair", Bp + 1), ("pair", 1)]
    return ([("0", n) for n in (1, B0 - 1, B0, B0 + 1, 4 * B0 + 3)] + [("pair", n) for n in (1, Bp - 1, Bp, Bp + 1, 4 * Bp + 3)]
            + [("indep", 2 * Bp + 1)])


_CASES = None


def cases():
    """name -> Case, in table order"""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = {}

    def add(name, desc, spec, routes=None, seed=0, M=1, nan_every=0, fn=None, matrix=None, entry="cov", placed=True):
        kernel = kernel_of(desc.size if matrix is None else matrix.shape[0], matrix is not None)
        if entry == "diff":
            kernel = "vals"
        levels = [_level(n, kind, 1000 * seed + 17 * l, M, nan_every, fn) for l, (kind, n) in enumerate(spec)]
        if placed:
            place(levels, desc, kernel)
        if routes is None:
            routes = ("direct", "lin") if lin_eligible(desc, matrix) else ("direct",)
        out[name] = Case(name, desc, levels, kernel, routes, matrix, entry)
        return out[name]

    # (at 49..64 moments MLMC_HIP_LINEARIZE_LEVEL0=0 also takes the row sums away: cov_rows requires lin0_eligible, api.hip)
    extra = {17: ("lin_cheb0", "lin_level0_0"), 49: ("lin_cheb0", "lin_rowsums0", "lin_level0_0"), 100: ("lin_cheb0",)}
    for R in LEGENDRE_R:
        d = ax.Desc(ax.LEGENDRE, R, DOM)
        routes = (("direct", "lin") if lin_eligible(d) else ("direct",)) + extra.get(R, ())
        k = kernel_of(R)
        spec = level_sizes(k) if R in FULL_R else level_sizes(k, short=True) + [("0", 4 * batches(k)[1] + 3), ("indep", 2 * batches(k)[0] + 1)]
        add("legendre_{}".format(R), d, spec, routes, seed=R)
    add("legendre_320", ax.Desc(ax.LEGENDRE, 320, DOM), level_sizes("vals", short=True), seed=320)
    for kernel, R in LONG_R.items():
        n = grid(kernel) * batches(kernel)[0] + batches(kernel)[0] + 5
        add("long_{}_{}".format(kernel, R), ax.Desc(ax.LEGENDRE, R, DOM), [("pair", n)], seed=400 + R)
    for R in FOURIER_R:
        add("fourier_{}".format(R), ax.Desc(ax.FOURIER, R, DOM), level_sizes(kernel_of(R)), seed=500 + R)
    for R in SPLINE_R:
        add("spline_{}".format(R), ax.Desc(ax.SPLINE, R, DOM), level_sizes(kernel_of(R)), seed=600 + R)
    for R in MONOMIAL_R:
        add("monomial_{}".format(R), ax.Desc(ax.MONOMIAL, R, MONO_DOM, MONO_REF), level_sizes(kernel_of(R)), seed=700 + R)
    for R in LOG_R:
        add("log_{}".format(R), ax.Desc(ax.LEGENDRE, R, LOG_DOM, log=True), level_sizes(kernel_of(R)), seed=800 + R,
            fn=lambda v: np.exp(0.9 * v))
    # safe_eval=False stays direct whatever the threshold says
    add("unclipped_20", ax.Desc(ax.LEGENDRE, 20, DOM, safe_eval=False), level_sizes("t2"), ("direct", "lin"), seed=20,
        fn=lambda v: np.clip(v, -3.96875, 3.96875))
    # the values route at a size whose long level stays affordable: 8 rows of 16 moments
    T = np.random.default_rng(816).normal(size=(8, 16)) / 4.0
    add("long_vals_8x16", ax.Desc(ax.LEGENDRE, 16, DOM), [("pair", grid("vals") * 64 + 64 + 5)], ("direct",), seed=816, matrix=T)
    # vector quantities with NaNs in one component only (shared mask)
    add("vector2_49", ax.Desc(ax.LEGENDRE, 49, DOM), level_sizes("t4", short=True) + [("pair", 131)], seed=249, M=2, nan_every=6)
    add("vector3_17", ax.Desc(ax.LEGENDRE, 17, DOM), level_sizes("t2", short=True) + [("pair", 515)], seed=317, M=3, nan_every=7)
    # a level whose every sample is dropped
    c = add("alldrop_33", ax.Desc(ax.LEGENDRE, 33, DOM), [("0", 70), ("pair", 40), ("pair", 70)], seed=933)
    c.levels[1][0][:] = np.nan
    # TransformedMoments: a seeded dense matrix; 70 rows of 80 and 130 rows of 130 (MODE_COV from values), and the variances of
    # MOMENTS mode through the difference Gram at 80 and 130 underlying moments
    for rows, cols in ((70, 80), (130, 130)):
        T = np.random.default_rng(rows).normal(size=(rows, cols)) / np.sqrt(cols)
        add("transformed_{}x{}".format(rows, cols), ax.Desc(ax.LEGENDRE, cols, DOM), level_sizes("vals"), ("direct",), seed=rows,
            matrix=T)
    for rows, cols in ((40, 80), (130, 130)):
        T = np.random.default_rng(7 * cols).normal(size=(rows, cols)) / np.sqrt(cols)
        add("diffgram_{}x{}".format(rows, cols), ax.Desc(ax.LEGENDRE, cols, DOM), level_sizes("vals"), ("direct",), seed=3 * cols,
            matrix=T, entry="diff")
    _CASES = out
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------
_REFERENCES, _LIN_SCALES, _TABLES = {}, {}, {}


def reference(case):
    """the long-double sums of a case (cov_exact.Sums), computed once"""
    if case.name not in _REFERENCES:
        if case.entry == "diff":
            _REFERENCES[case.name] = cx.diff_gram_sums(case.desc, case.levels, case.matrix)
        else:
            _REFERENCES[case.name] = cx.cov_sums(case.desc, case.levels, matrix=case.matrix)
    return _REFERENCES[case.name]


def lib_table(desc, squares):
    """mlmc_linearization_table of the library (host arithmetic only) [K, R, R]; squares: 0 products, 1 squares of Legendre /
    monomial sums, 2 / 3 the same for Chebyshev sums"""
    key = (desc.kind, desc.size, squares)
    if key not in _TABLES:
        from mlmc_amd import _lib
        R = desc.size
        K = 4 * R - 3 if squares in (1, 3) else 2 * R - 1
        t = np.empty(K * R * R)
        kind = _lib.LEGENDRE if desc.kind == ax.LEGENDRE else _lib.MONOMIAL
        _lib.check(_lib.load().mlmc_linearization_table(kind, R, squares, _lib.ptr(t), t.size))
        _TABLES[key] = cx.check_table(t.reshape(K, R, R))
    return _TABLES[key]


def lib_connection(m):
    """mlmc_chebyshev_connection_table of the library (host arithmetic only): T_j = sum_k b[j, k] P_k, [m, m]"""
    from mlmc_amd import _lib
    out = np.full(m * m, np.nan)
    _lib.check(_lib.load().mlmc_chebyshev_connection_table(m, _lib.ptr(out), out.size))
    return out.reshape(m, m)


def lin_scales(case, squares):
    """the linearised unit of every entry [L, M * R * R]: products (squares = 0) or squares (1), computed once"""
    key = (case.name, squares)
    if key not in _LIN_SCALES:
        _LIN_SCALES[key] = cx.lin_scales(case.desc, case.levels, lib_table(case.desc, squares))
    return _LIN_SCALES[key]


def judged(case, route, l, q):
    """(class key, reference values, scale) of quantity q ("s" | "sp") of level l under a route.  A linearised entry keeps the
    definition as its value and takes the linearised unit: the means of every level, and the second moments of the levels
    without coarse values where they need no matrix pass."""
    ref = reference(case)
    pair = case.levels[l][1] is not None
    lin = route.startswith("lin") and lin_eligible(case.desc, case.matrix)
    if lin and (q == "s" or (not pair and lin0(case, route))):
        scale = lin_scales(case, 0 if q == "s" else 1)[l]
        return (case.band, "lin", "pair" if pair else "0", q), getattr(ref, q)[l], scale
    return (case.band, "direct", "pair" if pair else "0", q), getattr(ref, q)[l], (ref.S if q == "s" else ref.SP)[l]


# ---------------------------------------------------------------------------------------------------------------------------
# tolerances
# ---------------------------------------------------------------------------------------------------------------------------
# Worst error of the fp64 twins against the long-double reference in units of 2^-53 * scale over every case of the class
# (band, route kind, "0" | "pair", quantity), measured and asserted by tests/test_cov_exact_cpu.py::test_twin_calibration_table.
# "direct": (A, B) = (the definition in fp64, the kernel's identities on rows with coefficients rounded beforehand);
# "lin": (A, B) = (extended Legendre / monomial sums contracted in ascending k, the same from Chebyshev sums | None).
COV_TWIN_UNITS = {
    ('diffgram', 'direct', '0', 's'): (4.02, 12.3),
    ('diffgram', 'direct', '0', 'sp'): (4.55, 7.91),
    ('diffgram', 'direct', 'pair', 's'): (0.12, 0.0851),
    ('diffgram', 'direct', 'pair', 'sp'): (2.43, 4.51),
    ('diffgram>128', 'direct', '0', 's'): (8.12, 22.3),
    ('diffgram>128', 'direct', '0', 'sp'): (7.12, 12.5),
    ('diffgram>128', 'direct', 'pair', 's'): (0.0891, 0.092),
    ('diffgram>128', 'direct', 'pair', 'sp'): (4.27, 5.48),
    ('fourier', 'direct', '0', 's'): (43.4, 8.81),
    ('fourier', 'direct', '0', 'sp'): (49.7, 15.2),
    ('fourier', 'direct', 'pair', 's'): (44.8, 8.32),
    ('fourier', 'direct', 'pair', 'sp'): (54.6, 36.3),
    ('legendre<=128', 'direct', '0', 's'): (178, 268),
    ('legendre<=128', 'direct', '0', 'sp'): (360, 536),
    ('legendre<=128', 'direct', 'pair', 's'): (1.04, 11.7),
    ('legendre<=128', 'direct', 'pair', 'sp'): (110, 183),
    ('legendre<=128', 'lin', '0', 's'): (134, 822),
    ('legendre<=128', 'lin', 'pair', 's'): (5.06, 8.87),
    ('legendre<=16', 'direct', '0', 's'): (8.65, 3.03),
    ('legendre<=16', 'direct', '0', 'sp'): (30.4, 10.9),
    ('legendre<=16', 'direct', 'pair', 's'): (0.947, 0.531),
    ('legendre<=16', 'direct', 'pair', 'sp'): (8.49, 3.36),
    ('legendre<=256', 'direct', '0', 's'): (213, 296),
    ('legendre<=256', 'direct', '0', 'sp'): (434, 592),
    ('legendre<=256', 'direct', 'pair', 's'): (1.59, 0.922),
    ('legendre<=256', 'direct', 'pair', 'sp'): (130, 283),
    ('legendre<=32', 'direct', '0', 's'): (38.4, 18.4),
    ('legendre<=32', 'direct', '0', 'sp'): (104, 49.7),
    ('legendre<=32', 'direct', 'pair', 's'): (8.94, 5.18),
    ('legendre<=32', 'direct', 'pair', 'sp'): (32, 21.7),
    ('legendre<=32', 'lin', '0', 's'): (7, 32),
    ('legendre<=32', 'lin', '0', 'sp'): (18, 52),
    ('legendre<=32', 'lin', 'pair', 's'): (2.63, 4.2),
    ('legendre<=512', 'direct', '0', 's'): (1.29e+03, 423),
    ('legendre<=512', 'direct', '0', 'sp'): (2.6e+03, 852),
    ('legendre<=512', 'direct', 'pair', 's'): (0.592, 0.345),
    ('legendre<=512', 'direct', 'pair', 'sp'): (778, 511),
    ('legendre<=64', 'direct', '0', 's'): (104, 126),
    ('legendre<=64', 'direct', '0', 'sp'): (230, 252),
    ('legendre<=64', 'direct', 'pair', 's'): (60.3, 59.7),
    ('legendre<=64', 'direct', 'pair', 'sp'): (170, 116),
    ('legendre<=64', 'lin', '0', 's'): (78, 166),
    ('legendre<=64', 'lin', '0', 'sp'): (112, 255),
    ('legendre<=64', 'lin', 'pair', 's'): (38.4, 144),
    ('log', 'direct', '0', 's'): (0.609, 0.609),
    ('log', 'direct', '0', 'sp'): (0.224, 0.224),
    ('log', 'direct', 'pair', 's'): (0.0381, 0.0381),
    ('log', 'direct', 'pair', 'sp'): (0.0373, 0.0373),
    ('log', 'lin', '0', 's'): (0.609, 0.885),
    ('log', 'lin', '0', 'sp'): (0.518, 0.52),
    ('log', 'lin', 'pair', 's'): (0.0763, 0.0767),
    ('monomial', 'direct', '0', 's'): (4.53, 4.53),
    ('monomial', 'direct', '0', 'sp'): (3.46, 3.46),
    ('monomial', 'direct', 'pair', 's'): (1.55, 1.21),
    ('monomial', 'direct', 'pair', 'sp'): (2.85, 4.08),
    ('monomial', 'lin', '0', 's'): (4.53, None),
    ('monomial', 'lin', '0', 'sp'): (3.42, None),
    ('monomial', 'lin', 'pair', 's'): (1.05, None),
    ('spline128', 'direct', '0', 's'): (1.44, 1.44),
    ('spline128', 'direct', '0', 'sp'): (1.94, 1.94),
    ('spline128', 'direct', 'pair', 's'): (0.42, 0.42),
    ('spline128', 'direct', 'pair', 'sp'): (1.86, 1.86),
    ('spline37', 'direct', '0', 's'): (1, 1),
    ('spline37', 'direct', '0', 'sp'): (2.11, 2.11),
    ('spline37', 'direct', 'pair', 's'): (0.315, 0.315),
    ('spline37', 'direct', 'pair', 'sp'): (2.03, 2.03),
    ('spline8', 'direct', '0', 's'): (0.355, 0.355),
    ('spline8', 'direct', '0', 'sp'): (0.221, 0.221),
    ('spline8', 'direct', 'pair', 's'): (0.252, 0.252),
    ('spline8', 'direct', 'pair', 'sp'): (0.0635, 0.0635),
    ('transformed', 'direct', '0', 's'): (3.94, 6.31),
    ('transformed', 'direct', '0', 'sp'): (1.09, 1.67),
    ('transformed', 'direct', 'pair', 's'): (0.0387, 0.03),
    ('transformed', 'direct', 'pair', 'sp'): (0.274, 0.323),
    ('transformed>128', 'direct', '0', 's'): (6.51, 12.5),
    ('transformed>128', 'direct', '0', 'sp'): (1.04, 2.14),
    ('transformed>128', 'direct', 'pair', 's'): (0.0493, 0.0337),
    ('transformed>128', 'direct', 'pair', 'sp'): (0.279, 0.709),
}


def tolerance(key):
    """max(16, 4 x the worse twin) units: the project's rule (tests/accum_cases.tolerance)"""
    a, b = COV_TWIN_UNITS[key]
    return max(16.0, 4.0 * max(a, b or 0.0))
