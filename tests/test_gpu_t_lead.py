"""GPU tests of the t box entries with a conditioned lead component (mlmc_copula_box_prob_tl_batch, mlmc_copula_box_draws_tl_batch,
DESIGN.md 3.5.27).  Every step of the header is held bit for bit against the elementwise entries that define it: the scale g0
against mlmc_chi2_conditional_scale, W0 against mlmc_student_t_cdf, the lead score against mlmc_student_t_quantile, the
conditioned scale against one NumPy expression, and the chain through the DIAGONAL IDENTITY: f[r, b, j] is W0 times the integrand
at point j of the Gaussian entry on the factor L[1:, 1:], the box (lo[1:] / sc_j, hi[1:] / sc_j) and the shift L_i0 y_0j.  Around it:
independence of batch / split / memory kind, repeatability, the closed forms down to marginal levels of 1e-12 with a cap on the
relative standard error, and the errors of the entries."""
import functools
import re

import numpy as np
import pytest

from tests import box_prob_cases as bc
from tests import t_box_cases as tb
from tests import t_lead_cases as tl
from tests.test_gpu_joint_samples import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
CLAMP_LO, CLAMP_HI = 2.0 ** -53, 1.0 - 2.0 ** -53
COND = dict(mixing="conditioned")


def _sd():
    from mlmc_amd.tool import simple_distribution
    return simple_distribution


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


class Case:
    def __init__(self, M, n, first, qmc, dof, seeds, B):
        self.M, self.n, self.first, self.qmc, self.dof, self.seeds, self.B = M, n, first, qmc, dof, tuple(seeds), B
        # box 0: a two-sided lead; box 1: an upper-tail lead with an infinite upper limit; box 2: an infinite lower limit;
        # box 3: a two-sided upper-tail lead and an EMPTY last component (for M = 1 that is an empty lead)
        self.L, self.lo, self.hi = tb.problem(M, B)

    def __repr__(self):
        return "M{}-n{}-{}-nu{:g}-R{}-B{}".format(self.M, self.n, "sobol" if self.qmc else "philox", self.dof, len(self.seeds), self.B)


# the shapes of tests/t_box_cases.SHAPES (M in {1, 2, 3, 12} and 128 once; Philox at first = 37 with n in {1, 27, 64, 200}; Sobol' with
# n in {64, 256}) with nu in {1, 3, 7.5, 64}, R in {1, 3} and B in {1, 4} spread over them
_EXTRA = ((1.0, (5,), 4), (3.0, (1, 2, 3), 1), (7.5, (4,), 4), (64.0, (0, 9, 11), 4), (3.0, (2,), 4),
          (7.5, (1, 2, 3), 4), (1.0, (6,), 4), (64.0, (3, 4, 5), 4), (3.0, (8,), 1))
CASES = tuple(Case(*shape, *extra) for shape, extra in zip(tb.SHAPES, _EXTRA))


@functools.lru_cache(maxsize=None)
def _prob(case):
    """(JointProbability, f [R, B, n], sc [R, B, n], v [R, B, n]) of the probability entry under default streams, once per case"""
    out = _sd().copula_box_probabilities(case.L, case.lo, case.hi, case.n, case.seeds, first=case.first, qmc=case.qmc, dof=case.dof,
                                         return_integrand=True, return_mixing=True, return_lead=True, **COND)
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _draws(case):
    return _sd().copula_box_draws(case.L, case.lo, case.hi, case.n, case.seeds, first=case.first, qmc=case.qmc, dof=case.dof,
                                  return_mixing=True, return_lead=True, **COND)


def _weights(case, b):
    """(a, bq, refl, d, e, W0) of box b from the device's own t CDF"""
    sd = _sd()
    with np.errstate(divide="ignore"):
        a, bq = case.lo[b, 0] / case.L[0, 0], case.hi[b, 0] / case.L[0, 0]
    refl = a > 0.0
    d, e = sd.student_t_cdf(np.array([-bq if refl else a, -a if refl else bq]), case.dof)
    return a, bq, refl, d, e, (e - d if a < bq else 0.0)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_lead_and_scale(hip, case):
    """steps 1 - 4: g0, W0, v and sc bit for bit from the elementwise entries"""
    sd = _sd()
    _, f, sc, v = _prob(case)
    R, B, n = len(case.seeds), case.B, case.n
    assert f.shape == sc.shape == v.shape == (R, B, n)
    for r, seed in enumerate(case.seeds):
        p0, w = tl.points_of(seed, case.M, case.first, n, case.qmc)
        g0 = sd.conditional_mixing_scale(p0, case.dof + 1.0)
        for b in range(B):
            a, bq, refl, d, e, W0 = _weights(case, b)
            p = np.minimum(np.maximum(d + w[0] * W0, bc.P_LO), bc.P_HI)
            want = sd.student_t_quantile(p, case.dof)
            want = -want if refl else want
            want = np.minimum(np.maximum(np.minimum(np.maximum(want, a), bq), -tl.V_CAP), tl.V_CAP)
            assert _same(v[r, b], want), (r, b)
            assert _same(sc[r, b], g0 * np.sqrt((case.dof + want * want) / (case.dof + 1.0))), (r, b)
            if a < bq:
                assert np.all((v[r, b] >= a) & (v[r, b] <= bq))
    assert np.all(np.isfinite(sc) & (sc > 0) & np.isfinite(v))
    # the draws entry sees the same scales and lead scores
    _, sc_d, v_d = _draws(case)
    assert _same(sc_d, sc) and _same(v_d, v)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_diagonal_identity(hip, case):
    """f[r, b, j] == W0 * (integrand of box j at point j of the Gaussian entry on L[1:, 1:], (lo[1:] / sc_j, hi[1:] / sc_j), the shift
    L_i0 y_0j and streams[1:]); for M = 1 f is W0 itself"""
    sd = _sd()
    res, f, sc, v = _prob(case)
    M = case.M
    with np.errstate(divide="ignore"):
        for r, seed in enumerate(case.seeds):
            for b in range(case.B):
                W0 = _weights(case, b)[5]
                if M == 1:
                    assert _same(f[r, b], np.full(case.n, W0)) and _same(res.replicates[r, b], W0)
                    continue
                lo_s, hi_s = case.lo[b][None, 1:] / sc[r, b][:, None], case.hi[b][None, 1:] / sc[r, b][:, None]      # [n, M - 1]
                y0 = v[r, b] / sc[r, b]
                shift = case.L[1:, 0][None, :] * y0[:, None]
                _, fg = sd.copula_box_probabilities(case.L[1:, 1:], lo_s, hi_s, case.n, [seed], shift=shift,
                                                    streams=list(range(2, M)), first=case.first, qmc=case.qmc, return_integrand=True)
                assert _same(f[r, b], W0 * np.diagonal(fg[0])), (r, b)
    assert np.all(np.isfinite(f) & (f >= 0) & (f <= 1))
    if case.B == 4:
        assert np.all(f[:, 3] == 0.0) and np.all(res.replicates[:, 3] == 0.0)               # an empty component or lead: exactly 0
        assert np.any(f[:, 1] > 0) and np.any(f[:, 2] > 0)                                  # infinite lead limits on either side


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_mean_is_the_tree_of_the_integrand(hip, case):
    res, f, _, _ = _prob(case)
    want = np.array([[bc.tree_mean(f[r, b], case.first, case.M) for b in range(case.B)] for r in range(len(case.seeds))])
    assert _same(res.replicates, want)
    assert _same(_sd().copula_box_probabilities(case.L, case.lo, case.hi, case.n, case.seeds, first=case.first, qmc=case.qmc,
                                                dof=case.dof, **COND).replicates, want)       # without the optional outputs


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_draws(hip, case):
    sd = _sd()
    res, f, sc, v = _prob(case)
    box = _draws(case)[0]
    R, B, M, n = len(case.seeds), case.B, case.M, case.n
    assert box.z.shape == (R, B, M, n) and box.u.shape == (R, B, M, n)
    assert _same(box.weights, f) and _same(box.prob.replicates, res.replicates)
    lo, hi = case.lo[None, :, :, None], case.hi[None, :, :, None]
    inside = np.broadcast_to(lo < hi, box.z.shape)
    assert np.all((box.z >= lo)[inside]) and np.all((box.z <= hi)[inside]) and np.all(np.isfinite(box.z[inside]))
    finite = np.isfinite(box.z)
    u = np.minimum(np.maximum(sd.student_t_cdf(np.where(finite, box.z, 0.0), case.dof), CLAMP_LO), CLAMP_HI)
    assert _same(box.u[finite], u[finite])
    with np.errstate(divide="ignore"):
        for r, seed in enumerate(case.seeds):
            for b in range(B):
                # the lead row: one rounded product, clipped
                assert _same(box.z[r, b, 0], np.minimum(np.maximum(v[r, b] * case.L[0, 0], case.lo[b, 0]), case.hi[b, 0]))
                if M == 1:
                    continue
                lo_s, hi_s = case.lo[b][None, 1:] / sc[r, b][:, None], case.hi[b][None, 1:] / sc[r, b][:, None]
                shift = case.L[1:, 0][None, :] * (v[r, b] / sc[r, b])[:, None]
                g = sd.copula_box_draws(case.L[1:, 1:], lo_s, hi_s, n, [seed], shift=shift, streams=list(range(2, M + 1)),
                                        first=case.first, qmc=case.qmc)
                zn = g.z[0][np.arange(n), :, np.arange(n)].T                                                    # [M - 1, n]
                want = np.minimum(np.maximum(zn * sc[r, b][None, :], case.lo[b][1:, None]), case.hi[b][1:, None])
                assert _same(box.z[r, b, 1:], want), (r, b)


def test_empty_lead(hip):
    sd = _sd()
    L = bc.chol_factor(3, 5)
    lo, hi = np.array([[0.5, -1.0, -1.0], [2.0, -1.0, -1.0]]), np.array([[-0.5, 1.0, 1.0], [2.0, 1.0, 1.0]])
    res, f = sd.copula_box_probabilities(L, lo, hi, 64, (1, 2), dof=3.0, return_integrand=True, **COND)
    assert np.all(f == 0.0) and np.all(res.replicates == 0.0) and np.all(res.prob == 0.0)
    box = sd.copula_box_draws(L, lo, hi, 64, (1, 2), dof=3.0, **COND)
    assert np.all(box.weights == 0.0) and np.all(box.z[:, :, 0] == hi[None, :, 0, None])


def test_independence_and_repeatability(hip, monkeypatch):
    import torch
    sd = _sd()
    for case in (CASES[2], CASES[6]):                                                       # Philox n = 200 at 37, Sobol' n = 256
        res, f, sc, v = _prob(case)
        box = _draws(case)[0]
        kw = dict(first=case.first, qmc=case.qmc, dof=case.dof, **COND)

        def prob(lo=case.lo, hi=case.hi, n=case.n, seeds=case.seeds, **more):
            args = dict(kw, return_integrand=True, return_mixing=True, return_lead=True)
            args.update(more)
            return sd.copula_box_probabilities(case.L, lo, hi, n, seeds, **args)

        def draws(lo=case.lo, hi=case.hi, n=case.n, seeds=case.seeds, **more):
            args = dict(kw, return_mixing=True, return_lead=True)
            args.update(more)
            return sd.copula_box_draws(case.L, lo, hi, n, seeds, **args)

        def host(x):
            return x.cpu().numpy() if isinstance(x, torch.Tensor) else x

        def check(p, d, rows=slice(None), boxes=slice(None), cols=slice(None)):
            assert _same(host(p[1]), f[rows, boxes, cols]) and _same(host(p[2]), sc[rows, boxes, cols])
            assert _same(host(p[3]), v[rows, boxes, cols])
            assert _same(host(d[0].weights), f[rows, boxes, cols]) and _same(host(d[0].z), box.z[rows, boxes, :, cols])
            assert _same(host(d[0].u), box.u[rows, boxes, :, cols]) and _same(host(d[1]), sc[rows, boxes, cols])
            assert _same(host(d[2]), v[rows, boxes, cols])

        p2, d2 = prob(), draws()
        check(p2, d2)                                                                       # a second run
        assert _same(p2[0].replicates, res.replicates) and _same(d2[0].prob.replicates, res.replicates)
        pd, dd = prob(device=True), draws(device=True)                                      # device outputs
        assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in (pd[1], pd[2], pd[3], dd[0].z, dd[0].u, dd[0].weights, dd[1], dd[2]))
        check(pd, dd)
        assert _same(pd[0].replicates, res.replicates) and _same(dd[0].prob.replicates, res.replicates)
        for pts in ("64", "130"):                                                           # the launch split
            monkeypatch.setenv("MLMC_BOX_PROB_BLOCK_POINTS", pts)
            ps, ds = prob(), draws()
            check(ps, ds)
            assert _same(ps[0].replicates, res.replicates) and _same(ds[0].prob.replicates, res.replicates)
            check(prob(device=True), draws(device=True))
        monkeypatch.delenv("MLMC_BOX_PROB_BLOCK_POINTS")
        for b in range(case.B):                                                             # calls split over boxes, seeds, ranges
            pb, db = prob(lo=case.lo[b], hi=case.hi[b]), draws(lo=case.lo[b], hi=case.hi[b])
            check(pb, db, boxes=slice(b, b + 1))
            assert _same(pb[0].replicates[:, 0], res.replicates[:, b])
        front = (99,) + case.seeds
        pf, df = prob(seeds=front), draws(seeds=front)
        check((pf[0], pf[1][1:], pf[2][1:], pf[3][1:]),
              (sd.BoxDraws(df[0].z[1:], df[0].u[1:], df[0].weights[1:], None), df[1][1:], df[2][1:]))
        assert _same(pf[0].replicates[1:], res.replicates)
        half = case.n // 2 - 3
        for c0, c1 in ((0, half), (half, case.n)):
            pr, dr = prob(n=c1 - c0, first=case.first + c0), draws(n=c1 - c0, first=case.first + c0)
            check(pr, dr, cols=slice(c0, c1))


# ---- closed forms: n = 2^12 Sobol' points, 8 seeds, 6 standard errors plus 1e-13, and the cap on the relative standard error ---------
ABS = 1e-13
CAP = 1.5


def _closed(kind, M, dof, level):
    sd = _sd()
    L = np.eye(M) if kind == "I" else bc.equicorrelation_factor(M)
    if level == "box":
        lo, hi = np.full(M, tl.TWO_SIDED[0]), np.full(M, tl.TWO_SIDED[1])
    else:
        lo, hi = np.full(M, tl.t_upper_quantile(dof, level)), np.full(M, np.inf)
    res = sd.copula_box_probabilities(L, lo, hi, tl.CLOSED_N, tl.CLOSED_SEEDS, dof=dof, **COND)
    exact = (tl.INDEPENDENT if kind == "I" else tl.EQUI)[(M, dof, level)]
    got, stderr = res.prob[0], res.stderr[0]
    twin_prob, twin_rel = tl.TWIN[(kind, M, dof, level)]
    print("{} M = {}, nu = {:g}, level {}: {:.9g} exact {:.9g}, off by {:.2f} stderr; rel. stderr {:.3g} (twin {:.3g})".format(
        kind, M, dof, level, got, exact, abs(got - exact) / stderr, stderr / got, twin_rel))
    assert abs(got - exact) <= 6.0 * stderr + ABS
    assert stderr / got <= CAP * twin_rel
    return stderr / got


@pytest.mark.parametrize("M", [2, 12])
@pytest.mark.parametrize("dof", tl.DOFS)
def test_closed_forms_independent(hip, M, dof):
    rel = {level: _closed("I", M, dof, level) for level in tl.LEVELS + ("box",)}
    # the relative-error property: the depth of the box does not cost accuracy
    twin_ratio = tl.TWIN[("I", M, dof, 1e-12)][1] / tl.TWIN[("I", M, dof, 1e-3)][1]
    assert rel[1e-12] / rel[1e-3] <= CAP * twin_ratio


@pytest.mark.parametrize("M", [2, 3])
def test_closed_forms_equicorrelated(hip, M):
    rel = {level: _closed("equi", M, 3.0, level) for level in tl.LEVELS}
    twin_ratio = tl.TWIN[("equi", M, 3.0, 1e-12)][1] / tl.TWIN[("equi", M, 3.0, 1e-3)][1]
    assert rel[1e-12] / rel[1e-3] <= CAP * twin_ratio


# ---- the errors of the entries ----------------------------------------------------------------------------------------------------
PROB, DRAWS = "mlmc_copula_box_prob_tl_batch", "mlmc_copula_box_draws_tl_batch"


def _raw(hip, entry, M=2, L=None, lo=(-1.0, -1.0), hi=(1.0, 1.0), dof=3.0, seeds=(0,), streams=None, mix=7, first=0, n=64, flags=8, kind=0):
    L = np.ascontiguousarray(np.eye(2) if L is None else L, dtype=np.float64)
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    B = lo.size // max(M, 1)
    seeds = np.asarray(seeds, dtype=np.uint64)
    streams = None if streams is None else np.asarray(streams, dtype=np.uint32)
    mean = np.full((seeds.size, B), -7.0)
    size = max(seeds.size * B * max(n, 0), 1)
    f, z = np.empty(size), np.empty(size * max(M, 1))
    if entry == PROB:
        rc = hip.lib().mlmc_copula_box_prob_tl_batch(M, hip.ptr(L), B, hip.ptr(lo), hip.ptr(hi), dof, seeds.size, hip.ptr(seeds),
                                                     hip.ptr(streams), mix, first, n, flags, hip.ptr(mean), None, None, None, kind)
    else:
        rc = hip.lib().mlmc_copula_box_draws_tl_batch(M, hip.ptr(L), B, hip.ptr(lo), hip.ptr(hi), dof, seeds.size, hip.ptr(seeds),
                                                      hip.ptr(streams), mix, first, n, flags, hip.ptr(mean), hip.ptr(f), hip.ptr(z), None,
                                                      None, None, kind)
    return rc, mean, hip.lib().mlmc_last_error().decode()


@pytest.mark.parametrize("entry", [PROB, DRAWS])
def test_errors_of_the_entry(hip, entry):
    rc, mean, _ = _raw(hip, entry)
    assert rc == 0 and 0 < mean[0, 0] < 1
    draws = entry == DRAWS
    big = bc.MAX_M + 1
    for kw, match in ((dict(dof=0.5), "dof must lie in"),
                      (dict(dof=64.5), "dof must lie in"),
                      (dict(dof=np.nan), "dof must lie in"),
                      (dict(mix=0), "mix_stream equals the stream of coordinate 0"),
                      (dict(streams=[5, 7]), "mix_stream equals the stream of coordinate 1") if draws else
                      (dict(streams=[7, 5]), "mix_stream equals the stream of coordinate 0"),
                      (dict(mix=1024), "mix_stream 1024 is not a Sobol' dimension"),
                      (dict(streams=[1024, 3]), "coordinate 0"),
                      (dict(M=big, L=np.eye(big), lo=[-1.0] * big, hi=[1.0] * big, mix=big), "cap"),
                      (dict(M=0), "M < 1"),
                      (dict(L=np.diag([1.0, 0.0])), "row 1"),
                      (dict(lo=[-1.0, np.nan]), "box 0, component 1"),
                      (dict(first=2 ** 52 - 63), "2\\^52"),
                      (dict(first=-1), "first"),
                      (dict(n=0), "n < 1"),
                      (dict(seeds=[]), "R < 1"),
                      (dict(flags=1), "ANTITHETIC"),
                      (dict(flags=2), "unknown"),
                      (dict(kind=5), "mem_kind")):
        rc, mean, msg = _raw(hip, entry, **kw)
        assert rc != 0 and re.search(match, msg) and msg.startswith(entry + ":"), (kw, msg)
        assert np.all(mean == -7.0)
    # the probability entry does not read streams[M - 1]: it may equal mix_stream
    assert (_raw(hip, entry, streams=[5, 7])[0] == 0) == (not draws)
    assert _raw(hip, entry, flags=0, mix=70000)[0] == 0
    assert _raw(hip, entry, first=2 ** 52 - 64)[0] == 0
