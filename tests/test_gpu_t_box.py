"""GPU tests of the Student-t box entries (mlmc_copula_box_prob_t_batch, mlmc_copula_box_draws_t_batch and the Python entries above
them).  The core check is the DIAGONAL IDENTITY: the integrand of the t entry at point j is, bit for bit, the integrand at point j of
the Gaussian entry called with the box (lo / s_j, hi / s_j) and the same chain streams; the only new arithmetic is two IEEE
divisions, so the accuracy of the t chain is that of the Gaussian chain, which tests/test_gpu_box_prob.py holds against mpmath.
Around it: the mixing scales and the draws bit for bit against the elementwise entries, the mean as the header's tree, independence
of batch / split / memory kind, repeatability, closed forms and the errors of the entries."""
import functools
import re

import numpy as np
import pytest
from scipy import special, stats

from tests import box_prob_cases as bc
from tests import t_box_cases as tb
from tests.test_gpu_joint_samples import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
CLAMP_LO, CLAMP_HI = 2.0 ** -53, 1.0 - 2.0 ** -53


def _sd():
    from mlmc_amd.tool import simple_distribution
    return simple_distribution


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


class Case:
    def __init__(self, M, n, first, qmc, dof, seeds, B):
        self.M, self.n, self.first, self.qmc, self.dof, self.seeds, self.B = M, n, first, qmc, dof, tuple(seeds), B
        self.L, self.lo, self.hi = tb.problem(M, B)

    def __repr__(self):
        return "M{}-n{}-{}-nu{:g}-R{}-B{}".format(self.M, self.n, "sobol" if self.qmc else "philox", self.dof, len(self.seeds), self.B)


# the shapes of tests/t_box_cases.SHAPES with nu in {1, 3, 7.5, 64}, R in {1, 3} and B in {1, 4} spread over them
_EXTRA = ((1.0, (5,), 4), (3.0, (1, 2, 3), 1), (7.5, (4,), 4), (64.0, (0, 9, 11), 4), (3.0, (2,), 1),
          (7.5, (1, 2, 3), 1), (1.0, (6,), 4), (64.0, (3, 4, 5), 4), (3.0, (8,), 1))
CASES = tuple(Case(*shape, *extra) for shape, extra in zip(tb.SHAPES, _EXTRA))


@functools.lru_cache(maxsize=None)
def _prob(case):
    """(JointProbability, f [R, B, n], s [R, n]) of the probability entry under default streams, computed once per case"""
    res, f, s = _sd().copula_box_probabilities(case.L, case.lo, case.hi, case.n, case.seeds, first=case.first, qmc=case.qmc, dof=case.dof,
                                               return_integrand=True, return_mixing=True)
    f.setflags(write=False)
    s.setflags(write=False)
    return res, f, s


@functools.lru_cache(maxsize=None)
def _draws(case):
    box, s = _sd().copula_box_draws(case.L, case.lo, case.hi, case.n, case.seeds, first=case.first, qmc=case.qmc, dof=case.dof,
                                    return_mixing=True)
    return box, s


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_mixing_scales(hip, case):
    sd = _sd()
    _, f, s = _prob(case)
    assert s.shape == (len(case.seeds), case.n) and f.shape == (len(case.seeds), case.B, case.n)
    for r, seed in enumerate(case.seeds):
        p0 = tb.mixing_points(seed, case.first, case.n, case.qmc)
        assert _same(s[r], sd.chi2_mixing_scale(p0, case.dof))
    assert np.all(np.isfinite(s) & (s > 0))
    # one scale per (seed, point) for every box of the call: a box alone, and the draws entry, see the same scales
    _, _, alone = sd.copula_box_probabilities(case.L, case.lo[-1], case.hi[-1], case.n, case.seeds, first=case.first, qmc=case.qmc,
                                              dof=case.dof, return_integrand=True, return_mixing=True)
    assert _same(alone, s) and _same(_draws(case)[1], s)
    # another mixing stream gives other scales
    if case.M <= 3:
        other = sd.copula_box_probabilities(case.L, case.lo, case.hi, case.n, case.seeds, first=case.first, qmc=case.qmc, dof=case.dof,
                                            mix_stream=9, return_mixing=True)[1]
        p0 = tb.mixing_points(case.seeds[0], case.first, case.n, case.qmc, stream=9)
        assert _same(other[0], sd.chi2_mixing_scale(p0, case.dof)) and not _same(other, s)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_diagonal_identity(hip, case):
    """f[r, b, j] of the t entry == f[j-th box, point j] of the Gaussian entry on the n boxes (lo / s_j, hi / s_j)"""
    sd = _sd()
    res, f, s = _prob(case)
    streams = tb.chain_streams(case.M)
    with np.errstate(divide="ignore"):
        for r, seed in enumerate(case.seeds):
            for b in range(case.B):
                lo_s, hi_s = case.lo[b][None, :] / s[r][:, None], case.hi[b][None, :] / s[r][:, None]           # [n, M]
                _, fg = sd.copula_box_probabilities(case.L, lo_s, hi_s, case.n, [seed], streams=streams, first=case.first,
                                                    qmc=case.qmc, return_integrand=True)
                assert _same(f[r, b], np.diagonal(fg[0]))
    assert np.all(np.isfinite(f) & (f >= 0) & (f <= 1))
    if case.B == 4:
        assert np.all(f[:, 3] == 0.0) and np.all(res.replicates[:, 3] == 0.0)               # the empty component: exactly 0
        assert np.any(np.isinf(case.hi[1])) and np.any(f[:, 1] > 0)                         # infinite limits stay infinite


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_mean_is_the_tree_of_the_integrand(hip, case):
    res, f, _ = _prob(case)
    # under the t law M = 1 uses its mixing point: the tree, as for every other M
    want = np.array([[bc.tree_mean(f[r, b], case.first) for b in range(case.B)] for r in range(len(case.seeds))])
    assert _same(res.replicates, want)
    assert _same(res.prob, res.replicates.mean(axis=0)) and res.n == case.n and np.array_equal(res.seeds, case.seeds)
    assert _same(_sd().copula_box_probabilities(case.L, case.lo, case.hi, case.n, case.seeds, first=case.first, qmc=case.qmc,
                                                dof=case.dof).replicates, want)               # without f_out and s_out


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_draws(hip, case):
    sd = _sd()
    res, f, s = _prob(case)
    box, _ = _draws(case)
    R, B, M, n = len(case.seeds), case.B, case.M, case.n
    assert box.z.shape == (R, B, M, n) and box.u.shape == (R, B, M, n)
    assert _same(box.weights, f) and _same(box.prob.replicates, res.replicates)
    lo, hi = case.lo[None, :, :, None], case.hi[None, :, :, None]
    inside = np.broadcast_to(lo < hi, box.z.shape)
    assert np.all((box.z >= lo)[inside]) and np.all((box.z <= hi)[inside]) and np.all(np.isfinite(box.z[inside]))
    assert np.all(np.broadcast_to(box.z == hi, box.z.shape)[~inside])
    finite = np.isfinite(box.z)
    u = np.minimum(np.maximum(sd.student_t_cdf(np.where(finite, box.z, 0.0), case.dof), CLAMP_LO), CLAMP_HI)
    assert _same(box.u[finite], u[finite])
    # the chain's normals are those of the Gaussian draws entry on the scaled boxes; the score is one rounded product, clipped
    streams = tb.chain_streams(M, draws=True)
    with np.errstate(divide="ignore"):
        for r, seed in enumerate(case.seeds):
            for b in range(B):
                lo_s, hi_s = case.lo[b][None, :] / s[r][:, None], case.hi[b][None, :] / s[r][:, None]
                g = sd.copula_box_draws(case.L, lo_s, hi_s, n, [seed], streams=streams, first=case.first, qmc=case.qmc)
                zn = g.z[0][np.arange(n), :, np.arange(n)].T                                                    # [M, n]: box j, point j
                want = np.minimum(np.maximum(zn * s[r][None, :], case.lo[b][:, None]), case.hi[b][:, None])
                assert _same(box.z[r, b], want)
                assert _same(box.weights[r, b], np.diagonal(g.weights[0]))


def test_independence_and_repeatability(hip, monkeypatch):
    import torch
    sd = _sd()
    for case in (CASES[2], CASES[6]):                                                       # Philox n = 200 at 37, Sobol' n = 256
        res, f, s = _prob(case)
        box, _ = _draws(case)
        kw = dict(first=case.first, qmc=case.qmc, dof=case.dof)

        def prob(lo=case.lo, hi=case.hi, n=case.n, seeds=case.seeds, **more):
            args = dict(kw, return_integrand=True, return_mixing=True)
            args.update(more)
            return sd.copula_box_probabilities(case.L, lo, hi, n, seeds, **args)

        def draws(lo=case.lo, hi=case.hi, n=case.n, seeds=case.seeds, **more):
            args = dict(kw, return_mixing=True)
            args.update(more)
            return sd.copula_box_draws(case.L, lo, hi, n, seeds, **args)

        def check(p, d, rows=slice(None), boxes=slice(None), cols=slice(None)):
            assert _same(p[1], f[rows, boxes, cols]) and _same(p[2], s[rows, cols])
            assert _same(d[0].weights, f[rows, boxes, cols]) and _same(d[0].z, box.z[rows, boxes, :, cols])
            assert _same(d[0].u, box.u[rows, boxes, :, cols]) and _same(d[1], s[rows, cols])

        p2, d2 = prob(), draws()
        check(p2, d2)                                                                       # a second run
        assert _same(p2[0].replicates, res.replicates) and _same(d2[0].prob.replicates, res.replicates)
        # device outputs
        pd, dd = prob(device=True), draws(device=True)
        assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in (pd[1], pd[2], dd[0].z, dd[0].u, dd[0].weights, dd[1]))
        check((pd[0], pd[1].cpu().numpy(), pd[2].cpu().numpy()),
              (sd.BoxDraws(dd[0].z.cpu().numpy(), dd[0].u.cpu().numpy(), dd[0].weights.cpu().numpy(), dd[0].prob), dd[1].cpu().numpy()))
        assert _same(pd[0].replicates, res.replicates) and _same(dd[0].prob.replicates, res.replicates)
        # the launch split
        for pts in ("64", "130"):
            monkeypatch.setenv("MLMC_BOX_PROB_BLOCK_POINTS", pts)
            ps, ds = prob(), draws()
            check(ps, ds)
            assert _same(ps[0].replicates, res.replicates) and _same(ds[0].prob.replicates, res.replicates)
            pd = prob(device=True)
            assert _same(pd[1].cpu().numpy(), f) and _same(pd[2].cpu().numpy(), s) and _same(pd[0].replicates, res.replicates)
            dd = draws(device=True)[0]
            assert _same(dd.z.cpu().numpy(), box.z) and _same(dd.u.cpu().numpy(), box.u)
        monkeypatch.delenv("MLMC_BOX_PROB_BLOCK_POINTS")
        # calls split over boxes, seeds and point ranges
        for b in range(case.B):
            pb, db = prob(lo=case.lo[b], hi=case.hi[b]), draws(lo=case.lo[b], hi=case.hi[b])
            check(pb, db, boxes=slice(b, b + 1))
            assert _same(pb[0].replicates[:, 0], res.replicates[:, b])
        front = (99,) + case.seeds
        pf, df = prob(seeds=front), draws(seeds=front)
        check((pf[0], pf[1][1:], pf[2][1:]), (sd.BoxDraws(df[0].z[1:], df[0].u[1:], df[0].weights[1:], None), df[1][1:]))
        assert _same(pf[0].replicates[1:], res.replicates)
        half = case.n // 2 - 3
        for c0, c1 in ((0, half), (half, case.n)):
            pr, dr = prob(n=c1 - c0, first=case.first + c0), draws(n=c1 - c0, first=case.first + c0)
            check(pr, dr, cols=slice(c0, c1))


# ---- closed forms: n = 2^12 Sobol' points, 8 seeds, 6 standard errors plus 1e-13 -----------------------------------------------------
CLOSED_N = 2 ** 12
ABS = 1e-13


def _gate(got, stderr, exact, what):
    print("{}: {:.12g} exact {:.12g}, off by {:.2f} stderr ({:.2g})".format(what, got, exact, abs(got - exact) / stderr, stderr))
    assert abs(got - exact) <= 6.0 * stderr + ABS, what


@pytest.mark.parametrize("dof", tb.DOFS)
def test_closed_form_one_component(hip, dof):
    sd = _sd()
    lo = np.array([[-1.0], [0.5], [-np.inf], [3.0]])
    hi = np.array([[0.25], [np.inf], [-2.0], [9.0]])
    res = sd.copula_box_probabilities([[1.0]], lo, hi, CLOSED_N, bc.SEEDS8, dof=dof)
    # the upper side through the lower tail of the mirrored limit, as the chain's reflection does
    exact = np.where(lo[:, 0] > 0, sd.student_t_cdf(-lo[:, 0], dof) - sd.student_t_cdf(-hi[:, 0], dof),
                     sd.student_t_cdf(hi[:, 0], dof) - sd.student_t_cdf(lo[:, 0], dof))
    for b in range(4):
        _gate(res.prob[b], res.stderr[b], exact[b], "nu = {:g}, ({:g}, {:g})".format(dof, lo[b, 0], hi[b, 0]))


@pytest.mark.parametrize("rho", [-0.5, 0.0, 0.7])
@pytest.mark.parametrize("dof", tb.DOFS)
def test_closed_form_orthant(hip, dof, rho):
    sd = _sd()
    L = np.linalg.cholesky(np.array([[1.0, rho], [rho, 1.0]]))
    h = sd.t_scores(special.ndtri(np.array([0.9, 0.99])), dof)
    res = sd.copula_box_probabilities(L, np.stack([h, h], axis=1), np.inf, CLOSED_N, bc.SEEDS8, dof=dof)
    for b, level in enumerate((0.9, 0.99)):
        _gate(res.prob[b], res.stderr[b], sd.bivariate_t_orthant(h[b], h[b], rho, dof), "nu = {:g}, rho = {:g}, level {:g}".format(dof, rho, level))


def test_identical_components(hip):
    """rho = 0.999999 and the same limit in both components: the one-dimensional value.  The two-dimensional orthant falls short of
    it by P(Y1 > h, Y2 < h) = pdf(h) sqrt(1 - rho^2) E[Z+] to first order (Y2 - Y1 = sqrt(1 - rho^2) Z near the limit), 5.6e-4 pdf(h);
    the limit 8.4 at nu = 64 is where that is below 1e-14, a tenth of the absolute part of the gate (a probability of 3e-12).  At a
    small nu such a limit lies where only the mixing variable reaches, which 2^12 points do not resolve"""
    sd = _sd()
    rho, dof, h = 0.999999, 64.0, 8.4
    assert stats.t.pdf(h, dof) * np.sqrt(1.0 - rho * rho) * 0.4 < 0.1 * ABS
    L = np.linalg.cholesky(np.array([[1.0, rho], [rho, 1.0]]))
    res = sd.copula_box_probabilities(L, [h, h], np.inf, CLOSED_N, bc.SEEDS8, dof=dof)
    assert res.prob[0] > 0
    _gate(res.prob[0], res.stderr[0], float(sd.student_t_cdf(-h, dof)), "rho = 0.999999")


# ---- the errors of the entries ----------------------------------------------------------------------------------------------------
def _raw(hip, entry, M=2, L=None, lo=(-1.0, -1.0), hi=(1.0, 1.0), dof=3.0, seeds=(0,), streams=None, mix=7, first=0, n=64, flags=8, kind=0):
    L = np.ascontiguousarray(np.eye(2) if L is None else L, dtype=np.float64)
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    B = lo.size // max(M, 1)
    seeds = np.asarray(seeds, dtype=np.uint64)
    streams = None if streams is None else np.asarray(streams, dtype=np.uint32)
    mean = np.full((seeds.size, B), -7.0)
    size = max(seeds.size * B * max(n, 0), 1)
    f, z = np.empty(size), np.empty(size * max(M, 1))
    if entry == "mlmc_copula_box_prob_t_batch":
        rc = hip.lib().mlmc_copula_box_prob_t_batch(M, hip.ptr(L), B, hip.ptr(lo), hip.ptr(hi), dof, seeds.size, hip.ptr(seeds), hip.ptr(streams),
                                                    mix, first, n, flags, hip.ptr(mean), None, None, kind)
    else:
        rc = hip.lib().mlmc_copula_box_draws_t_batch(M, hip.ptr(L), B, hip.ptr(lo), hip.ptr(hi), dof, seeds.size, hip.ptr(seeds),
                                                     hip.ptr(streams), mix, first, n, flags, hip.ptr(mean), hip.ptr(f), hip.ptr(z), None, None,
                                                     kind)
    return rc, mean, hip.lib().mlmc_last_error().decode()


@pytest.mark.parametrize("entry", ["mlmc_copula_box_prob_t_batch", "mlmc_copula_box_draws_t_batch"])
def test_errors_of_the_entry(hip, entry):
    rc, mean, _ = _raw(hip, entry)
    assert rc == 0 and 0 < mean[0, 0] < 1
    draws = entry.endswith("draws_t_batch")
    big = bc.MAX_M + 1
    for kw, match in ((dict(dof=0.5), "dof must lie in"),
                      (dict(dof=64.5), "dof must lie in"),
                      (dict(dof=np.nan), "dof must lie in"),
                      (dict(mix=0), "mix_stream equals the stream of coordinate 0"),
                      (dict(streams=[5, 7] if draws else [7]), "mix_stream equals the stream of coordinate {}".format(1 if draws else 0)),
                      (dict(mix=1024), "mix_stream 1024 is not a Sobol' dimension"),
                      (dict(streams=[1024, 3] if draws else [1024]), "coordinate 0"),
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
    # Philox takes any uint32 stream for the mixing variable; the last point of the sequence
    assert _raw(hip, entry, flags=0, mix=70000)[0] == 0
    assert _raw(hip, entry, first=2 ** 52 - 64)[0] == 0
