"""The case table of the extended-precision checks of the accumulation kernels, shared by tests/test_accum_exact_cpu.py
(calibration of the fp64 twins) and tests/test_gpu_accum_exact.py (the device).  Plain NumPy data: nothing here touches the
device or the package."""
import numpy as np

from tests import accum_exact as ax
from tests.util import level_arrays

# sizes of the levels: one sample; around one wave; around two waves with a one-sample pair level; a ragged many-block level
# with a five-sample one; more than one trip of every workgroup (4099 = 16 * 256 + 3)
SIZES = ([1], [63, 64, 65], [127, 129, 1], [257, 1000, 5], [4099, 513, 2])
DEVICE_SIZES = [257, 1000, 5]             # the size list that also runs from device-resident tensors in one launch
STEPS = [0.5, 0.1, 0.03]

DOM = (-4.0, 4.0)                         # power-of-two ends: x -> t is exact for the hand-placed values
MONO_DOM = (-4.0, 4.5)
LOG_DOM = (0.05, 30.0)
COMPONENT_DOMS = ((-4.0, 4.0), (-3.0, 3.5), (-5.0, 4.25))

# wide, exact tiles, PLAIN third-wave limit | term split | compile-time windows | run-time windows
LEGENDRE_VAR_R = (1, 3, 16, 17, 28, 29, 48, 49, 60, 64, 65, 100, 128, 129, 130, 320, 512)
LEGENDRE_MEAN_ONLY_R = (65, 127, 128, 129, 200, 256)      # one window | second window; sp = NaN
MONOMIAL_R = (8, 33, 52)
FOURIER_R = (9, 33, 128)
SPLINE_R = (8, 37, 128)
COV_R = (5, 17, 33, 64)
COV_SIZES = ([257, 1000, 5], [65, 64, 1])
COMPONENT_K = ((ax.LEGENDRE, 5), (ax.LEGENDRE, 33), (ax.LEGENDRE, 64), (ax.MONOMIAL, 8))


def legendre_band(R):
    for top in (16, 48, 64, 128, 256, 512):
        if R <= top:
            return "legendre<={}".format(top)
    raise ValueError(R)


def _inv(desc, r):
    """raw value of the reference coordinate r, in fp64"""
    lin = (r - desc.ref_domain[0]) / desc.scale + desc.shift
    return float(np.exp(lin)) if desc.log else float(lin)


def spline_fill(desc):
    """One ordinary value in every third knot span (0.40625 of the way through it).  Every B-spline is supported on four spans,
    so each row sees at least one of them at a value of 0.01 or more: a row whose only sample lies 1e-3 of a span inside its
    support, B ~ (u ns - k)^3 / 6, carries the rounding of u ns at 3000 times its weight in any fp64 evaluation, and the
    condition scale sum |phi| does not describe that.  With these values no row of a level of 63 or more samples is in that
    position, whatever the seeded data does."""
    ns = desc.size - 3
    return [8.0 * ((k + 0.40625) / ns) - 4.0 for k in range(0, ns, 3)]


def edge_pairs(desc):
    """Hand-placed (fine, coarse) pairs of one level.  First a pair with fine == coarse, then both ends against each other (on
    DOM: t = +1 / -1 exactly), then every special value once as the fine and once as the coarse value of a pair with an ordinary
    value: the ends, the two doubles next to each of them inside (on DOM: x = 4 (1 - 2^-53), which the fp64 transform rounds to
    t = 1, then t = 1 - 2^-52; t = -1 + 2^-53, -1 + 2^-52), +-0.0 (log: 0 and -1, dropped), one ulp outside each end (the upper
    one on DOM is KEPT by the reference's arithmetic: x + 4 rounds to 8) and a NaN.  safe_eval=False: no value outside.

    Splines add values exactly on interior knots (t = fl(k / ns); first two, middle, last two) -- a B-spline whose support begins
    or ends at a knot is ~1e-45 at the fp64 value of that knot -- and the values of spline_fill, paired with each other.

    The two ordinary values sit at the fractions 0.618... (golden ratio) and 0.414... (sqrt 2 - 1) of the reference domain: k
    times them stays away from every multiple of half a Fourier period for all k <= 64, and they are not mirror images of each
    other (a dyadic fraction made cos(16 t) = 1 to rounding, the pair 0.618 / 0.382 made every cosine row cancel)."""
    a, b = desc.domain
    w = desc.ref_domain[1] - desc.ref_domain[0]
    same = _inv(desc, desc.ref_domain[0] + 0.6180339887498949 * w)
    mid = _inv(desc, desc.ref_domain[0] + 0.41421356237309515 * w)
    lo1, hi1 = np.nextafter(a, np.inf), np.nextafter(b, -np.inf)
    special = [b, a, hi1, np.nextafter(hi1, -np.inf), lo1, np.nextafter(lo1, np.inf)]
    special += [0.0, -1.0] if desc.log else [0.0, -0.0]
    if desc.safe_eval:
        special += [np.nextafter(b, np.inf), np.nextafter(a, -np.inf)]
    special.append(np.nan)
    if desc.kind == ax.SPLINE:
        assert desc.domain == DOM and not desc.log
        ns = desc.size - 3
        for k in sorted({1, 2, ns // 2, ns - 2, ns - 1}):             # t = fl(k / ns) exactly: (x + 4) / 8 is exact
            special.append(8.0 * (k / ns) - 4.0)
    pairs = [(same, same), (b, a), (a, b)]
    if desc.kind == ax.FOURIER:
        # sin(k t) is ~1e-14 at both ends and its error is k t 2^-53 in any evaluation: the head of the list, which is all that a
        # level of two or five samples holds, takes the ordinary values instead
        pairs = [(same, same), (mid, same), (same, mid), (b, a), (a, b)]
    for v in special:
        pairs += [(float(v), mid), (mid, float(v))]
    if desc.kind == ax.SPLINE:
        fill = spline_fill(desc)
        pairs += [(fill[i], fill[i + 1] if i + 1 < len(fill) else mid) for i in range(0, len(fill), 2)]
    return pairs


def level_pairs(desc, paired):
    """the list a level takes: edge_pairs; level 0 has fine values only and takes the two ends, then every distinct value of
    edge_pairs once"""
    if paired:
        return edge_pairs(desc)
    out, seen = [], set()
    pairs = edge_pairs(desc)
    for v in [desc.domain[0], desc.domain[1]] + [vf for vf, _ in pairs] + [vc for _, vc in pairs]:
        key = np.float64(v).tobytes()
        if key not in seen:
            seen.add(key)
            out.append((v, None))
    return out


def place_edges(levels, descs):
    """Overwrite samples of every level with the hand-placed pairs.  A level shorter than the list takes its head -- a pair level
    the pair with fine == coarse first (a one-sample level then consists of exact zeros), then the ends; level 0 the ends first.
    At t = +-1 every Legendre polynomial is +-1, so the condition scale sum |phi_k| of a level of two or five samples is at least
    1 in every row: a single ordinary sample lies next to a zero of some P_k (k < 512) and would put that row's scale, and with
    it the unit of the whole class, a factor of a thousand below its error.  descs: one per component row (its own values, at its
    own sample positions) -- or one desc for all rows, the pairs then go round the rows."""
    for f, c in levels:
        M, n = f.shape
        for m in range(M if len(descs) > 1 else 1):
            pairs = level_pairs(descs[m], c is not None)
            assert n < 63 or len(pairs) <= n - 2
            step = max(1, (n - 2) // len(pairs))
            for i, (vf, vc) in enumerate(pairs[:n]):
                pos = (min(1, n - 1) + i * step + m) % n
                row = m if len(descs) > 1 else i % M
                f[row, pos] = vf
                if c is not None:
                    c[row, pos] = vc
    return levels


class Case:
    """name; cls = the tolerance class; descs (one, or one per component for the per-component entries); levels
    [(fine [M, n], coarse [M, n] | None)]; entry: "var" | "mean_only" (LevelAccumulator MOMENTS) | "cov" (MODE_COV, means only) |
    "component" (mlmc_accum_estimate_multi_var and mlmc_accum_estimate_multi); device: also run from device-resident tensors;
    parity: a case on which the new tolerance is shown to imply the 1e-10 gate (every family and size with variances, on the
    largest size list)"""

    def __init__(self, name, cls, descs, levels, entry="var", device=False, parity=False):
        self.name, self.cls, self.descs, self.levels, self.entry = name, cls, list(descs), levels, entry
        self.device, self.parity = device, parity
        self.desc = self.descs[0]
        self.M = levels[0][0].shape[0]
        self.L = len(levels)

    def __repr__(self):
        return self.name


def _data(sizes, M=1, nan_every=0, seed=1234, fn=None):
    levels = level_arrays(sizes, STEPS[:len(sizes)], M, nan_every, seed=seed)
    out = []
    for f, c in levels:
        f = np.ascontiguousarray(f if fn is None else fn(f))
        c = None if c is None else np.ascontiguousarray(c if fn is None else fn(c))
        out.append((f, c))
    return out


def _tag(sizes):
    return "x".join(str(n) for n in sizes)


_CASES = None


def cases():
    """name -> Case, in table order"""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = {}

    def add(name, cls, descs, levels, **kw):
        out[name] = Case(name, cls, descs, place_edges(levels, descs), **kw)

    def family(kind, Rs, dom, cls_of, entry="var"):
        for R in Rs:
            for sizes in SIZES:
                d = ax.Desc(kind, R, dom)
                add("{}{}_{}_{}".format(kind, "_mean" if entry == "mean_only" else "", R, _tag(sizes)), cls_of(R), [d],
                    _data(sizes, seed=1234 + R), entry=entry, device=(sizes == DEVICE_SIZES),
                    parity=(entry == "var" and sizes == SIZES[-1]))

    family(ax.LEGENDRE, LEGENDRE_VAR_R, DOM, legendre_band)
    family(ax.LEGENDRE, LEGENDRE_MEAN_ONLY_R, DOM, legendre_band, entry="mean_only")
    family(ax.MONOMIAL, MONOMIAL_R, MONO_DOM, lambda R: "monomial")
    family(ax.FOURIER, FOURIER_R, DOM, lambda R: "fourier")
    family(ax.SPLINE, SPLINE_R, DOM, lambda R: "spline{}".format(R))
    # the general (non-PLAIN) loop: a vector quantity with NaNs (mask kernel), log, safe_eval=False
    for R in (17, 64):
        for sizes in ([257, 1000, 5], [63, 64, 65]):
            add("vector3_{}_{}".format(R, _tag(sizes)), legendre_band(R), [ax.Desc(ax.LEGENDRE, R, DOM)],
                _data(sizes, M=3, nan_every=7, seed=77 + R), device=(sizes == DEVICE_SIZES))
    for R in (20, 50):
        for sizes in ([257, 1000, 5], [127, 129, 1]):
            add("log_{}_{}".format(R, _tag(sizes)), "log", [ax.Desc(ax.LEGENDRE, R, LOG_DOM, log=True)],
                _data(sizes, seed=99 + R, fn=lambda v: np.exp(0.9 * v)), device=(sizes == DEVICE_SIZES))
    for sizes in ([257, 1000, 5], [63, 64, 65]):
        add("unclipped_8_{}".format(_tag(sizes)), legendre_band(8), [ax.Desc(ax.LEGENDRE, 8, DOM, safe_eval=False)],
            _data(sizes, seed=8, fn=lambda v: np.clip(v, -3.96875, 3.96875)), device=(sizes == DEVICE_SIZES))
    # the per-component entries: three domains, every component masked on its own
    for kind, K in COMPONENT_K:
        descs = [ax.Desc(kind, K, dom) for dom in COMPONENT_DOMS]
        add("component_{}_{}".format(kind, K), legendre_band(K) if kind == ax.LEGENDRE else "monomial", descs,
            _data(DEVICE_SIZES, M=3, nan_every=11, seed=500 + K), entry="component", device=True)
    # covariance means on the direct route (chunks far below the size from which the library linearises)
    for R in COV_R:
        for sizes in COV_SIZES:
            add("cov_{}_{}".format(R, _tag(sizes)), legendre_band(R), [ax.Desc(ax.LEGENDRE, R, DOM)],
                _data(sizes, seed=300 + R), entry="cov")
    _CASES = out
    return out


def component_levels(case, m):
    """the [1, n] rows of component m of a per-component case"""
    return [(f[m:m + 1], None if c is None else c[m:m + 1]) for f, c in case.levels]


def sums_of(case, dtype=ax.LD, variant="A"):
    """What the entry of `case` must return, in `dtype`: an ax.Sums with n, n_rm [L] and s, sp, S, SP [L, K].  "component":
    n, n_rm [L, M] and s ... [L, M, K], every component from its own desc and its own keep rule.  "cov": s, S are the
    covariance means [L, R * R] and their scales (sp, SP: None -- the covariance variances, every size, route and kernel of the
    covariance, are judged by tests/cov_exact.py with the cases of tests/cov_cases.py)."""
    if case.entry == "component":
        per = [ax.level_sums(d, component_levels(case, m), dtype, variant) for m, d in enumerate(case.descs)]
        out = ax.Sums()
        out.n, out.n_rm = np.stack([p.n for p in per], axis=1), np.stack([p.n_rm for p in per], axis=1)
        for key in ("s", "sp", "S", "SP"):
            setattr(out, key, np.stack([getattr(p, key) for p in per], axis=1))
        return out
    out = ax.level_sums(case.desc, case.levels, dtype, variant, keep_rows=(case.entry == "cov"))
    if case.entry == "cov":
        out.s, out.S = ax.cov_sums(out.phi)
        out.sp = out.SP = None
    out.phi = None
    return out


_REFERENCES = {}


def reference(case):
    """the long-double sums of a case, computed once"""
    if case.name not in _REFERENCES:
        _REFERENCES[case.name] = sums_of(case)
    return _REFERENCES[case.name]


def quantities(case):
    """the judged outputs of a case -> key of TWIN_UNITS"""
    return {"cov": ("cov_s",), "mean_only": ("s",)}.get(case.entry, ("s", "sp"))


def judged(sums, quantity):
    """(values, scales) of a quantity in an ax.Sums"""
    return (sums.sp, sums.SP) if quantity == "sp" else (sums.s, sums.S)


# ---------------------------------------------------------------------------------------------------------------------------
# the evaluation-only path (Moments.eval_all)
# ---------------------------------------------------------------------------------------------------------------------------
EVAL_CASES = {"legendre_512": (ax.LEGENDRE, 512), "fourier_128": (ax.FOURIER, 128), "spline_128": (ax.SPLINE, 128)}


def eval_desc(name):
    kind, R = EVAL_CASES[name]
    return ax.Desc(kind, R, DOM)


def eval_points(name):
    """the hand-placed values of edge_pairs (NaN and the values outside included) and a 1501-point grid over the domain"""
    d = eval_desc(name)
    vals = [v for pair in edge_pairs(d) for v in pair]
    grid = np.linspace(d.domain[0], d.domain[1], 1501)
    grid[0], grid[-1] = d.domain
    return np.concatenate([np.array(vals, dtype=np.float64), grid])


# ---------------------------------------------------------------------------------------------------------------------------
# tolerances
# ---------------------------------------------------------------------------------------------------------------------------
# Worst error of the fp64 twins (A: the reference's operation order; B: coefficients rounded beforehand) against the
# long-double reference, in units of 2^-53 * condition scale, over every case of the class.  Measured and asserted by
# tests/test_accum_exact_cpu.py::test_twin_calibration_table; (A, B), B = None where the family has one twin.
TWIN_UNITS = {
    "legendre<=16": dict(s=(3.44, 2.0), sp=(4.6, 1.43), cov_s=(4.15, 4.15)),
    "legendre<=48": dict(s=(24.0, 44.0), sp=(24.6, 29.3), cov_s=(50.2, 25.6)),
    "legendre<=64": dict(s=(34.1, 63.0), sp=(50.5, 42.3), cov_s=(88.3, 72.6)),
    "legendre<=128": dict(s=(64.3, 143.0), sp=(59.1, 95.4)),
    "legendre<=256": dict(s=(210.0, 328.0), sp=(61.1, 101.0)),
    "legendre<=512": dict(s=(1530.0, 683.0), sp=(1210.0, 455.0)),
    "monomial": dict(s=(4.39, None), sp=(1.39, None)),
    "fourier": dict(s=(129.0, 28.6), sp=(200.0, 51.1)),
    "spline8": dict(s=(6.71, None), sp=(55.7, None)),
    "spline37": dict(s=(112.0, None), sp=(96.0, None)),
    "spline128": dict(s=(305.0, None), sp=(242.0, None)),
    "log": dict(s=(0.327, 0.327), sp=(0.303, 0.295)),
}

# The same for Moments.eval_all on eval_points(), unit 2^-53 * max(|value|, 1), worst over all points and terms.
EVAL_TWIN_UNITS = {
    "legendre_512": (4240.0, 1860.0),
    "fourier_128": (256.0, 44.1),
    "spline_128": (109.0, None),
}


def tolerance(cls, quantity):
    """max(16, 4 x max(twin A, twin B)) units: the margin of 4 and the floor of 16 of tests/maxent_cases.py.  The kernels sum
    in another order and run their own recurrences; a recurrence with precomputed coefficients carries one coefficient rounding
    for every sample alike, which adds up linearly where the integer coefficients of legvander average out -- twin B measures
    that effect from the textbook recurrences, without restating the device's."""
    a, b = TWIN_UNITS[cls][quantity]
    return max(16.0, 4.0 * max(a, b or 0.0))


def eval_tolerance(name):
    a, b = EVAL_TWIN_UNITS[name]
    return 4.0 * max(a, b or 0.0)
