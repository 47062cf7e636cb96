"""GPU tests of the batched divergences between max-entropy densities (k_q_divergences in mlmc_amd/csrc/density.hip) through the public
entries: simple_distribution.divergences, SimpleDistribution / Distribution.divergence, Estimate.bootstrap_component_divergences
and mlmc_density_divergences_batch.

The six columns (include/mlmc_hip.h) are finite sums; tests/divergence_cases.py evaluates them in 80-bit long double.  The main test
requires |value - reference| <= tol_units 2^-53 scale, tol_units = 4 x the worst error of the fp64 twin on the CPU
(dc.TWIN_UNITS_D, tests/test_divergence_cpu.py), at least 16.  The worst units per tolerance class and column are printed before
the assertion (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

from tests import divergence_cases as dc
from tests import maxent_cases as mc
from tests import maxent_exact as mx
from tests import quantile_cases as qc
from tests.test_gpu_quantiles import _dist
from tests.test_gpu_tail_means import _gaussian, estimate      # noqa: F401 (estimate: the fixture of the Estimate-level test)

pytestmark = pytest.mark.gpu
LD = np.longdouble
Q_TABLE_BYTES = 64 << 20                                            # density.hip


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


def _columns(distrs, first, second, lo, hi, quad=None):
    """mlmc_density_divergences_batch itself: out [P, 6]"""
    from mlmc_amd import _lib
    from mlmc_amd.tool import simple_distribution as sd
    handles, r1, lam, sig = sd._batch_problem_args(distrs)
    a = np.array([float(d.domain[0]) for d in distrs])
    b = np.array([float(d.domain[1]) for d in distrs])
    first, second = np.ascontiguousarray(first, dtype=np.int32), np.ascontiguousarray(second, dtype=np.int32)
    lo = None if lo is None else np.ascontiguousarray(lo, dtype=np.float64)
    hi = None if hi is None else np.ascontiguousarray(hi, dtype=np.float64)
    quad = (distrs[0].n_intervals, distrs[0]._gauss_degree) if quad is None else quad
    out = np.full((len(first), 6), -7.0)
    _lib.check(_lib.lib().mlmc_density_divergences_batch(len(distrs), C.cast(handles, C.c_void_p), _lib.ptr(r1), _lib.ptr(lam),
                                                         _lib.ptr(sig), _lib.ptr(a), _lib.ptr(b), quad[0], quad[1], len(first),
                                                         _lib.ptr(first), _lib.ptr(second), _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(out)))
    return out


class _Problems:
    """distribution objects of (case, multipliers, rule), one per distinct problem, and the index arrays of a list of pairs"""

    def __init__(self):
        self.index, self.distrs = {}, []

    def of(self, case, lam, quad):
        key = (case.name, np.asarray(lam, dtype=np.float64).tobytes(), quad)
        if key not in self.index:
            self.index[key] = len(self.distrs)
            self.distrs.append(_dist(case, lam, quad))
        return self.index[key]

    def dist(self, case, lam, quad):
        return self.distrs[self.of(case, lam, quad)]


@pytest.fixture(scope="module")
def table(hip):
    """the pair table (dc.pairs at fp64 Newton multipliers) with its long-double reference, and ONE call of the entry per rule over
    all its pairs, shared by the tests"""
    out, every = [], dc.pairs()
    for quad in qc.RULES:
        group = [p for p in every if p.quad == quad]
        probs = _Problems()
        first = [probs.of(p.prior[0], p.prior[1], quad) for p in group]
        second = [probs.of(p.posterior[0], p.posterior[1], quad) for p in group]
        lo, hi = [p.interval[0] for p in group], [p.interval[1] for p in group]
        got = _columns(probs.distrs, first, second, lo, hi)
        refs = [p.reference() for p in group]
        out.append(dict(quad=quad, pairs=group, probs=probs, first=np.array(first), second=np.array(second), lo=np.array(lo),
                        hi=np.array(hi), got=got, refs=refs))
    return out


def test_accuracy(table):
    """all six columns of every pair of the table against the long-double reference"""
    failures, worst = [], {}
    for t in table:
        assert len(t["probs"].distrs) < 2 * len(t["pairs"])              # problems are shared between the pairs
        for p, got, (ref, scale) in zip(t["pairs"], t["got"], t["refs"]):
            tol = dc.divergence_tolerance(p.cls)
            u = dc.units(got, ref, scale)
            for c in range(6):
                key = (p.cls, dc.COLUMNS[c])
                if u[c] > worst.get(key, (-1.0, None))[0]:
                    worst[key] = (float(u[c]), p.tag)
                if not u[c] <= tol:
                    failures.append(f"{p.tag}: {dc.COLUMNS[c]} is {u[c]:.4g} units off (tolerance {tol:g})")
    print()
    for (cls, col), (v, where) in sorted(worst.items()):
        print(f"worst {cls:8s} {col:7s} {v:10.4g} units at {where} (twin {dc.TWIN_UNITS_D[cls]:g})")
    assert not failures, "\n".join(failures)


def test_identical_pairs(table):
    """a problem against itself: four exact zeros and bit-equal masses, through the array call and the method"""
    n = 0
    for t in table:
        for p, got in zip(t["pairs"], t["got"]):
            if p.same:
                n += 1
                assert np.all(got[:4] == 0.0) and got[dc.MASS_P] == got[dc.MASS_Q] and got[dc.MASS_P] > 0, p.tag
                d = t["probs"].dist(p.prior[0], p.prior[1], p.quad)
                res = d.divergence(d)
                assert res.kl == 0.0 and res.l2 == 0.0 and res.tv == 0.0 and res.hellinger == 0.0, p.tag
                assert res.mass_prior == res.mass_posterior == got[dc.MASS_P], p.tag
    assert n >= 2 * len(dc.SELF_CASES)


RULES_ODD_EVEN = ((1, 1), (1, 4), (7, 5), (7, 21), (64, 1), (64, 4), (200, 5))


def test_mass_is_the_mass_of_the_cdf_entry(table):
    """on the prior's whole domain MASS_P is bit for bit the mass of cdfs_on_rule / mlmc_density_cdf_batch for the same problem
    and rule (and MASS_Q the posterior's, where the interval is its domain): on the two rules of the table, and on rules with 1, 7,
    64 and 200 cells of 1, 4, 5 and 21 nodes (odd and even node counts: the last node alone, or none)"""
    from mlmc_amd.tool import simple_distribution as sd
    n = 0
    for t in table:
        distrs = t["probs"].distrs
        mass = sd._on_rule(distrs, [np.array([0.5])] * len(distrs), False, "cdfs_on_rule")[1]
        for p, got, i, j in zip(t["pairs"], t["got"], t["first"], t["second"]):
            if p.interval == p.prior[0].domain:
                n += 1
                assert got[dc.MASS_P] == mass[i], p.tag
            if p.interval == p.posterior[0].domain:
                assert got[dc.MASS_Q] == mass[j], p.tag
    assert n >= 3 * len(mc.cases())
    t = table[0]
    sel = [k for k, p in enumerate(t["pairs"]) if "converged / perturbed" in p.tag or "mix_R9 converged / fourier" in p.tag
           or "monomial_R6 converged / spline" in p.tag]
    for quad in RULES_ODD_EVEN:
        probs = _Problems()
        first = [probs.of(t["pairs"][k].prior[0], t["pairs"][k].prior[1], quad) for k in sel]
        second = [probs.of(t["pairs"][k].posterior[0], t["pairs"][k].posterior[1], quad) for k in sel]
        got = _columns(probs.distrs, first, second, None, None)
        mass = sd._on_rule(probs.distrs, [np.array([0.5])] * len(probs.distrs), False, "cdfs_on_rule")[1]
        assert np.array_equal(got[:, dc.MASS_P], mass[first]) and np.array_equal(got[:, dc.MASS_Q], mass[second]), quad
        # and the other columns against the reference on this rule, for the cross-family pairs and two more (fewer nodes than on the
        # rules of the calibration, so sums of fewer terms: the tolerance of the class holds a fortiori)
        for k, row in zip(sel, got):
            p = t["pairs"][k]
            if p.prior[0].name in ("mix_R9", "monomial_R6", "norm12_R21", "fourier_R9"):
                ref, scale = dc.pair_sums(p.prior, p.posterior, p.interval, quad)
                u = dc.units(row, ref, scale)
                assert np.all(u <= dc.divergence_tolerance(p.cls)), (p.tag, quad, u)


def test_batch_independence(table):
    """each pair alone, in the full batch, in a permuted batch and with its problems shared by many pairs: the same bits; NULL
    intervals are the intersections; the `divergence` method is the P = 1 call"""
    from mlmc_amd.tool import simple_distribution as sd
    from mlmc_amd.tool.distribution import Distribution
    rng = np.random.default_rng(3)
    for t in table:
        distrs, first, second, lo, hi, got = t["probs"].distrs, t["first"], t["second"], t["lo"], t["hi"], t["got"]
        P = len(first)
        assert np.array_equal(_columns(distrs, first, second, None, None), got, equal_nan=True)       # the table's intervals are those
        perm = rng.permutation(P)
        assert np.array_equal(_columns(distrs, first[perm], second[perm], lo[perm], hi[perm]), got[perm])
        # every pair three times, the problems in reverse order
        rev = len(distrs) - 1 - np.arange(len(distrs))
        many = _columns([distrs[i] for i in rev], np.tile(rev[first], 3), np.tile(rev[second], 3), np.tile(lo, 3), np.tile(hi, 3))
        assert np.array_equal(many, np.tile(got, (3, 1)))
        for k in range(0, P, 5):
            alone = _columns([distrs[first[k]], distrs[second[k]]], [0], [1], lo[k:k + 1], hi[k:k + 1])
            assert np.array_equal(alone[0], got[k]), t["pairs"][k].tag
        # the Python entries: roots of two columns, the rest as it is
        res = sd.divergences([distrs[i] for i in first], [distrs[j] for j in second], np.stack([lo, hi], axis=1))
        want = got.copy()
        want[:, 1], want[:, 3] = np.sqrt(got[:, 1]), np.sqrt(got[:, 3])
        assert np.array_equal(np.stack(res, axis=1), want)
        for k in (0, P // 2, P - 1):
            one = distrs[second[k]].divergence(distrs[first[k]], interval=(lo[k], hi[k]))
            assert isinstance(one, sd.Divergences) and all(isinstance(v, float) for v in one) and np.array_equal(np.array(one), want[k])
            assert np.array_equal(np.array(distrs[second[k]].divergence(distrs[first[k]])), want[k])
    t = table[0]
    k = [i for i, p in enumerate(t["pairs"]) if p.tag.startswith("norm12_R21 converged / perturbed")][0]
    p = t["pairs"][k]
    old_prior = _dist(p.prior[0], p.prior[1], p.quad, Distribution)
    old_post = _dist(p.posterior[0], p.posterior[1], p.quad, Distribution)
    got = np.array(old_post.divergence(old_prior))
    assert got[0] == t["got"][k][0] and got[1] == np.sqrt(t["got"][k][1]) and got[4] == t["got"][k][4]
    # a sub-interval: inside both domains, another value than on the whole domain
    a, b = p.interval
    sub = np.array(old_post.divergence(old_prior, interval=(a + 0.25 * (b - a), b - 0.25 * (b - a))))
    assert 0 < sub[4] < got[4] and 0 < sub[0] != got[0]


def test_rules_bit_for_bit(table):
    """rules with 1, 7, 64 and 200 cells of 1, 5 and 21 nodes (and 4: no odd node): a pair alone == the pair in the batch"""
    t = table[0]
    sel = list(range(0, len(t["pairs"]), 9)) + [k for k, p in enumerate(t["pairs"]) if " / " in p.tag and "spline" in p.tag]
    for n_int in (1, 7, 64, 200):
        for deg in (1, 4, 5, 21):
            quad = (n_int, deg)
            probs = _Problems()
            first = [probs.of(t["pairs"][k].prior[0], t["pairs"][k].prior[1], quad) for k in sel]
            second = [probs.of(t["pairs"][k].posterior[0], t["pairs"][k].posterior[1], quad) for k in sel]
            lo, hi = t["lo"][sel], t["hi"][sel]
            got = _columns(probs.distrs, first, second, lo, hi)
            assert np.all(np.isfinite(got)) and np.all(got[:, 4:] > 0), quad
            for i in range(0, len(sel), 3):
                alone = _columns([probs.distrs[first[i]], probs.distrs[second[i]]], [0], [1], lo[i:i + 1], hi[i:i + 1])
                assert np.array_equal(alone[0], got[i]), (quad, t["pairs"][sel[i]].tag)
            back = _columns(probs.distrs[::-1], len(probs.distrs) - 1 - np.array(first)[::-1], len(probs.distrs) - 1 - np.array(second)[::-1],
                            lo[::-1], hi[::-1])
            assert np.array_equal(back[::-1], got), quad


def test_groups_of_the_table_bound(hip):
    """Gaussian problems on a rule of 2^18 cells: a pair's table row is 6 x 2^18 doubles = 12 MiB, the bound of 64 MiB puts 5 pairs
    into a group, so 6 pairs run in two groups; each is bit for bit the pair alone"""
    n_int = 1 << 18
    per_group = Q_TABLE_BYTES // (8 * 6 * n_int)
    P = per_group + 1
    assert per_group == 5
    distrs = [_gaussian(0.25 * k - 0.5, 1.0 + 0.125 * k, n_intervals=n_int) for k in range(P + 1)]
    first, second = np.arange(P), np.arange(P) + 1
    got = _columns(distrs, first, second, None, None)
    assert np.all(np.isfinite(got)) and np.all(got[:, :4] > 0)
    for k in (0, per_group - 1, per_group):
        alone = _columns([distrs[k], distrs[k + 1]], [0], [1], None, None)
        assert np.array_equal(alone[0], got[k]), k
    # the densities are exp(-z^2 / 2) on mu +- 8 sigma: masses sqrt(2 pi) sigma, up to the truncation of the narrower domain
    # (Phi(-8 sigma_narrow / sigma) >= Phi(-8) = 6e-16 of it) and the recursive summation of N = 2^18 x 21 terms, 2 (N + 8) 2^-53
    for k in range(P):
        for col, d in ((dc.MASS_P, distrs[k]), (dc.MASS_Q, distrs[k + 1])):
            sigma = (d.domain[1] - d.domain[0]) / 16
            assert abs(got[k, col] / (np.sqrt(2 * np.pi) * sigma) - 1) <= 1e-3, (k, col)
    wide = _columns(distrs[:2], [1], [0], None, None)[0]                     # the narrower domain inside the wider: its whole mass
    sigma0 = (distrs[0].domain[1] - distrs[0].domain[0]) / 16
    assert abs(wide[dc.MASS_Q] / (np.sqrt(2 * np.pi) * sigma0) - 1) <= 2 * (n_int * 21 + 8) * 2.0 ** -53 + 2e-15


# ---- closed form ------------------------------------------------------------------------------------------------------------------
EXP_DOMAIN = (-4.0, 4.0)
# (lambda_0, lambda_1) of prior and posterior.  Legendre on (-4, 4): t = x / 4, density exp(-l0 - l1 x / 4): slopes 0.5 / 0.25 and
# 0.5 / -0.375 per unit of x.  Monomial (ref_domain (0, 1)): t = (x + 4) / 8, slopes 0.25 / 0.125 and 0.25 / 0.0625.  In the first pair
# of each family q > p on the whole domain; in the second the densities cross at x = 0, which is the edge of cell 32 of the 64-cell
# rule, so |q - p| is smooth on every cell.
EXP_PAIRS = ((mx.LEGENDRE, (1.0, 2.0), (-0.5, 1.0)), (mx.LEGENDRE, (1.0, 2.0), (1.0, -1.5)),
             (mx.MONOMIAL, (1.5, 2.0), (0.5, 1.0)), (mx.MONOMIAL, (1.0, 2.0), (1.75, 0.5)))


def _exponential(kind, lam):
    """(case, c0, c1): the density exp(-(c0 + c1 x)), c0 / c1 in long double from the transform of the family"""
    desc = mx.Desc(kind, 2, EXP_DOMAIN)
    case = mc.Case(f"exp_{kind}", desc, np.array([1.0, 0.0]), np.ones(2), np.array(lam), "other")
    scale, shift, ref0 = LD(desc.scale), LD(desc.shift), LD(desc.ref_domain[0])
    l0, l1 = LD(lam[0]), LD(lam[1])                                  # t = (x - shift) scale + ref0
    return case, l0 + l1 * (ref0 - shift * scale), l1 * scale


def _exp_integral(c0, c1, lo, hi, power=0):
    """int_lo^hi x^power exp(-(c0 + c1 x)) dx, power 0 or 1, in long double"""
    lo, hi = LD(lo), LD(hi)
    if c1 == 0:
        return np.exp(-c0) * ((hi - lo) if power == 0 else (hi * hi - lo * lo) / 2)
    el, eh = np.exp(-(c0 + c1 * lo)), np.exp(-(c0 + c1 * hi))
    if power == 0:
        return (el - eh) / c1
    return (lo * el - hi * eh) / c1 + (el - eh) / (c1 * c1)


def test_exponential_closed_form(hip):
    """R1 = 2: p = exp(-(a0 + a1 x)), q = exp(-(b0 + b1 x)) have elementary integrals for all six columns.  The truncation error of
    the 21-point rule on cells of width 1/8 at these slopes (below 0.5 per unit: (0.5 / 8)^42 / 42!) is far below one unit, so the
    tolerance is the unit tolerance of the accuracy test."""
    lo, hi = EXP_DOMAIN
    for kind, lam_p, lam_q in EXP_PAIRS:
        (cp, a0, a1), (cq, b0, b1) = _exponential(kind, lam_p), _exponential(kind, lam_q)
        mp, mq = _exp_integral(a0, a1, lo, hi), _exp_integral(b0, b1, lo, hi)
        # int p (log p - log q) = int p ((b0 - a0) + (b1 - a1) x)
        kl = (b0 - a0) * mp + (b1 - a1) * _exp_integral(a0, a1, lo, hi, 1) - mp + mq
        l2sq = _exp_integral(2 * a0, 2 * a1, lo, hi) - 2 * _exp_integral(a0 + b0, a1 + b1, lo, hi) + _exp_integral(2 * b0, 2 * b1, lo, hi)
        h2 = (mp + mq) / 2 - _exp_integral((a0 + b0) / 2, (a1 + b1) / 2, lo, hi)
        cross = (b0 - a0) / (a1 - b1)                                  # p = q there
        if lo < cross < hi:
            assert cross == 0
            left = _exp_integral(b0, b1, lo, 0.0) - _exp_integral(a0, a1, lo, 0.0)
            right = _exp_integral(b0, b1, 0.0, hi) - _exp_integral(a0, a1, 0.0, hi)
            assert left * right < 0
            tv = (abs(left) + abs(right)) / 2
        else:
            tv = abs(mq - mp) / 2
        want = np.array([kl, l2sq, tv, h2, mp, mq], dtype=LD)
        dp, dq = _dist(cp, cp.lam0, (64, 21)), _dist(cq, cq.lam0, (64, 21))
        got = _columns([dp, dq], [0], [1], None, None)[0]
        _, scale = dc.pair_sums((cp, cp.lam0), (cq, cq.lam0), EXP_DOMAIN, (64, 21))
        u = dc.units(got, want, scale)
        print(f"\nexponential {kind} {lam_p} / {lam_q}: units {np.round(u, 3)} values {got}")
        assert np.all(u <= dc.divergence_tolerance("regular")), (kind, lam_p, lam_q, u)
        res = dq.divergence(dp)
        assert res.kl == got[0] and res.l2 == np.sqrt(got[1]) and res.hellinger == np.sqrt(got[3])


# ---- specials ---------------------------------------------------------------------------------------------------------------------
def test_clipped_pairs(table):
    """mc.clip_multipliers against their negatives, against the converged multipliers and the other way round: finite or inf exactly
    where the reference is, and within the tolerance where finite"""
    t = table[0]
    n_inf = 0
    for name in mc.CLIP_CASES:
        case = mc.cases()[name]
        lam = [p.prior[1] for p in t["pairs"] if p.tag.startswith(f"{name} converged / perturbed")][0]
        lc = mc.clip_multipliers(case, lam)
        for prior, posterior in (((case, lc), (case, -lc)), ((case, lc), (case, lam)), ((case, lam), (case, lc))):
            exps = []
            ref, scale = dc.pair_sums(prior, posterior, case.domain, t["quad"], exponents=exps)
            mc.assert_clip_band(exps[0])
            mc.assert_clip_band(exps[1])
            dc.assert_overflow_band(exps[2])
            got = _columns([_dist(*prior, t["quad"]), _dist(*posterior, t["quad"])], [0], [1], None, None)[0]
            assert np.array_equal(np.isfinite(got), np.isfinite(ref)) and np.array_equal(got[~np.isfinite(ref)], ref[~np.isfinite(ref)].astype(float))
            n_inf += int(np.isinf(got[dc.L2SQ]))
            u = dc.units(got, ref, scale)
            assert np.all(u <= dc.divergence_tolerance("regular")), (name, u)
    assert n_inf == len(mc.CLIP_CASES)


def test_nan_rows(table):
    """NaN multipliers and a distribution domain wider than the basis' domain: six NaNs for the pairs that use the problem, the
    other pairs of the call as before, no error"""
    t = table[0]
    k = [i for i, p in enumerate(t["pairs"]) if p.tag.startswith("mix_R9 converged / perturbed")][0]
    p = t["pairs"][k]
    good_p, good_q = _dist(p.prior[0], p.prior[1], p.quad), _dist(p.posterior[0], p.posterior[1], p.quad)
    bad = p.prior[1].copy()
    bad[2] = np.nan
    nan_lam = _dist(p.prior[0], bad, p.quad)
    wide = _dist(p.prior[0], p.prior[1], p.quad)
    wide.domain = (p.prior[0].domain[0] - 1.0, p.prior[0].domain[1])
    distrs = [good_p, good_q, nan_lam, wide]
    first, second = [0, 2, 0, 3, 0], [1, 1, 2, 3, 1]
    a, b = p.prior[0].domain
    lo, hi = [a, a, a, a - 1.0, a], [b] * 5
    got = _columns(distrs, first, second, lo, hi)
    for row in (0, 4):
        assert np.array_equal(got[row], t["got"][k])
    assert np.all(np.isnan(got[1:4]))
    # on the intersection of the domains the wide distribution is the good one
    assert np.array_equal(_columns(distrs, [3], [1], None, None)[0], t["got"][k])
    from mlmc_amd.tool import simple_distribution as sd
    res = sd.divergences([good_p, nan_lam], [nan_lam, nan_lam])
    assert all(np.all(np.isnan(v)) for v in res)


def test_argument_errors(hip):
    from mlmc_amd import Legendre
    lib = hip.lib()
    name = "mlmc_density_divergences_batch"
    fn = getattr(lib, name)
    B, P = 4, 5
    doms = [(-2.0, 2.0), (-2.0, 2.0), (-1.0, 3.0), (2.0, 5.0)]
    fns = [Legendre(5, dom) for dom in doms]
    handles = (C.c_void_p * B)(*[f._basis_handle().value for f in fns])
    hp = C.cast(handles, C.c_void_p)
    r1 = np.full(B, 5, dtype=np.int32)
    lam, sig = np.zeros((B, 5)), np.ones((B, 5))
    lam[:, 0] = np.log(4.0)
    a, b = np.array([d[0] for d in doms]), np.array([d[1] for d in doms])
    first, second = np.array([0, 1, 0, 2, 2], dtype=np.int32), np.array([1, 0, 2, 0, 3], dtype=np.int32)
    lo, hi = np.array([-2.0, -1.0, -1.0, 0.0, 2.0]), np.array([2.0, 1.0, 2.0, 0.5, 3.0])
    out = np.empty((P, 6))
    Pt = hip.ptr

    def call(**kw):
        v = dict(B=B, h=hp, r1=r1, lam=lam, sig=sig, a=a, b=b, ni=0, deg=0, P=P, first=first, second=second, lo=lo, hi=hi, out=out)
        v.update(kw)
        return fn(v["B"], v["h"], Pt(v["r1"]), Pt(v["lam"]), Pt(v["sig"]), Pt(v["a"]), Pt(v["b"]), v["ni"], v["deg"], v["P"],
                  Pt(v["first"]), Pt(v["second"]), Pt(v["lo"]), Pt(v["hi"]), Pt(v["out"]))

    def expect(rc, pattern):
        with pytest.raises(hip.MlmcHipError, match=pattern):
            hip.check(rc)
    assert call() == 0
    # uniform densities 1/4: zero distances, masses = width / 4
    assert np.all(out[:, :4] == 0.0) and np.all(np.abs(out[:, 4] - (hi - lo) / 4) < 1e-14) and np.array_equal(out[:, 4], out[:, 5])
    out[:] = -1.0
    assert call(lo=None, hi=None) == 0                             # the intersections
    assert np.all(np.abs(out[:, 4] - np.array([4.0, 4.0, 3.0, 3.0, 1.0]) / 4) < 1e-14)
    for key in ("r1", "lam", "sig", "a", "b", "first", "second", "out"):
        expect(call(**{key: None}), name + ".*null")
    expect(call(h=None), name + ".*null")
    expect(call(lo=None), name + ": lo and hi must both")
    expect(call(hi=None), name + ": lo and hi must both")
    expect(call(B=-1), name + ".*B < 0")
    expect(call(P=-1), name + ".*P < 0")
    expect(call(deg=65), name + ".*gauss_degree")
    expect(call(deg=-1), name + ".*gauss_degree")
    expect(call(ni=-1), name + ".*n_intervals")
    expect(call(ni=(1 << 20) + 1), name + ".*n_intervals")
    # errors of one problem name the problem
    bad_b = b.copy(); bad_b[2] = a[2]
    expect(call(b=bad_b), name + ": problem 2.*domain")
    nan_a = a.copy(); nan_a[0] = np.nan
    expect(call(a=nan_a), name + ": problem 0.*domain")
    bad_r1 = r1.copy(); bad_r1[1] = 6
    expect(call(r1=bad_r1), name + ": problem 1.*R1")
    from mlmc_amd.engine import _IdentityBasis
    id_h = (C.c_void_p * B)(*[f._basis_handle().value for f in fns])
    id_h[1] = _IdentityBasis()._basis_handle().value
    id_r1 = r1.copy(); id_r1[1] = 1
    expect(call(h=C.cast(id_h, C.c_void_p), r1=id_r1), name + ": problem 1.*unsupported basis kind")
    # errors of one pair name the pair
    for arr, key in ((first, "first"), (second, "second")):
        for bad_index in (-1, B):
            bad = arr.copy(); bad[3] = bad_index
            expect(call(**{key: bad}), name + ": pair 3: problem index outside")
    for k, (l, h) in ((1, (1.0, 1.0)), (2, (1.0, 0.5)), (0, (np.nan, 1.0)), (4, (2.0, np.inf))):
        bad_lo, bad_hi = lo.copy(), hi.copy()
        bad_lo[k], bad_hi[k] = l, h
        expect(call(lo=bad_lo, hi=bad_hi), name + f": pair {k}: the interval must be finite with lo < hi")
    for k, (l, h) in ((2, (-1.5, 2.0)), (2, (-1.0, 2.5)), (4, (1.5, 3.0)), (0, (-2.0, np.nextafter(2.0, 3.0)))):
        bad_lo, bad_hi = lo.copy(), hi.copy()
        bad_lo[k], bad_hi[k] = l, h
        expect(call(lo=bad_lo, hi=bad_hi), name + f": pair {k}: the interval is not inside both domains")
    apart = second.copy(); apart[1] = 3                              # (-2, 2) and (2, 5) touch in one point
    expect(call(second=apart, lo=None, hi=None), name + ": pair 1: the two domains do not intersect")
    # no-ops
    out[:] = 7.25
    assert fn(0, None, None, None, None, None, None, 0, 0, P, Pt(first), Pt(second), None, None, Pt(out)) == 0
    assert call(P=0) == 0 and call(P=0, first=None, second=None, out=None) == 0
    assert np.all(out == 7.25)


# ---- Estimate ---------------------------------------------------------------------------------------------------------------------
def test_bootstrap_component_divergences(hip, estimate):
    from mlmc_amd.estimator import DivergenceSpread, divergence_upper
    from mlmc_amd.tool import simple_distribution as sd
    st, q, fns, est, dens = estimate
    M, B, R = len(fns), 8, 9
    one = est.bootstrap_component_divergences(B, seed=7, level=0.8, moments_fns=fns, densities=dens)
    two = est.bootstrap_component_divergences(B, seed=7, level=0.8, densities=dens)
    assert isinstance(one, DivergenceSpread) and one.seed == 7
    for x, y in zip(one, two):
        assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)
    for v in (one.kl, one.l2, one.tv, one.hellinger):
        assert v.shape == (B, M) and np.all(v[one.success] > 0)
    assert one.success.shape == (B, M) and one.success.dtype == bool and np.array_equal(one.n_ok, one.success.sum(axis=0)) and one.n_ok.min() > 0
    assert one.upper.shape == (M, 4)
    assert np.array_equal(one.upper, divergence_upper((one.kl, one.l2, one.tv, one.hellinger), one.success, 0.8))
    assert np.all(one.upper[:, 0] <= np.max(np.where(one.success, one.kl, 0), axis=0))
    # the same replicate densities as the quantile bands: the same verdicts
    bq = est.bootstrap_component_quantiles(np.array([0.05, 0.5, 0.95]), B, seed=7, moments_fns=fns, densities=dens)
    assert np.array_equal(one.success, bq.success)
    # the same chain from public pieces
    reps = est.est_bootstrap_components(B, moments_fns=fns, seed=7)
    distrs = []
    for b in range(B):
        for m in range(M):
            mobj = dens[m][3]
            mu = np.sum([reps.l_means[b, l, m, :R] @ mobj._base_matrix.T for l in range(reps.l_means.shape[1])], axis=0)
            distrs.append(sd.SimpleDistribution(mobj, np.stack((mu, np.ones(mobj.size)), axis=1), domain=mobj.domain))
    results = sd.estimate_densities_minimize(distrs, 1e-8, 0.0)
    assert np.array_equal(np.array([bool(r.success) for r in results]).reshape(B, M), one.success)
    res = sd.divergences([dens[m][0] for _ in range(B) for m in range(M)], distrs)
    for got, want in zip((one.kl, one.l2, one.tv, one.hellinger), (res.kl, res.l2, res.tv, res.hellinger)):
        assert np.array_equal(got, want.reshape(B, M))
    # a replicate of a few thousand samples stays close to the estimate: total variation well below 1/2
    assert np.all(one.tv[one.success] < 0.25) and np.all(one.hellinger[one.success] < 0.5)
    assert np.all(np.abs(res.mass_prior - 1) < 1e-4) and np.all(np.abs(res.mass_posterior[one.success.reshape(-1)] - 1) < 1e-4)
