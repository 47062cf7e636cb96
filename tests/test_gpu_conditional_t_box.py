"""GPU tests of the conditional box entries of the Student-t copula (mlmc_copula_box_prob_tc_batch, mlmc_copula_box_draws_tc_batch
and conditional_box_probabilities / conditional_box_draws above them).  The core check is the DIAGONAL IDENTITY: the integrand at
point j is, bit for bit, the integrand at point j of the Gaussian entry called with the box ((lo - shift) / c_j, (hi - shift) / c_j),
c_j = scale * s_j, and the same chain streams; the new arithmetic is one subtraction, one product and one IEEE division, which NumPy
reproduces, so the accuracy is that of the Gaussian chain, which tests/test_gpu_box_prob.py holds against mpmath.  Around it: the
mixing scales against mlmc_chi2_conditional_scale, the reduction to the t entries, the draws, the mean as the header's tree,
independence of batch / split / memory kind, repeatability and the errors of the entries."""
import functools
import re

import numpy as np
import pytest

from tests import box_prob_cases as bc
from tests import conditional_t_box_cases as ctc
from tests import t_box_cases as tb
from tests.test_gpu_joint_samples import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
CLAMP_LO, CLAMP_HI = 2.0 ** -53, 1.0 - 2.0 ** -53
CASES = ctc.CASES


def _sd():
    from mlmc_amd.tool import simple_distribution
    return simple_distribution


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _kw(case):
    return dict(dof_mix=case.dof_mix, shift=case.shift, scale=case.scale, first=case.first, qmc=case.qmc)


@functools.lru_cache(maxsize=None)
def _prob(case):
    """(JointProbability, f [R, B, n], s [R, n]) of the probability entry under default streams, computed once per case"""
    res, f, s = _sd().conditional_box_probabilities(case.L, case.lo, case.hi, case.n, case.seeds, case.dof, return_integrand=True,
                                                    return_mixing=True, **_kw(case))
    f.setflags(write=False)
    s.setflags(write=False)
    return res, f, s


@functools.lru_cache(maxsize=None)
def _draws(case):
    box, s = _sd().conditional_box_draws(case.L, case.lo, case.hi, case.n, case.seeds, case.dof, return_mixing=True, **_kw(case))
    for a in (box.z, box.u, box.weights, s):
        a.setflags(write=False)
    return box, s


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_mixing_scales(hip, case):
    sd = _sd()
    _, f, s = _prob(case)
    assert s.shape == (len(case.seeds), case.n) and f.shape == (len(case.seeds), case.B, case.n)
    for r, seed in enumerate(case.seeds):
        p0 = tb.mixing_points(seed, case.first, case.n, case.qmc)
        assert _same(s[r], sd.conditional_mixing_scale(p0, case.dof_mix))
    assert np.all(np.isfinite(s) & (s > 0))
    # one scale per (seed, point) for every box of the call: a box alone, and the draws entry, see the same scales
    kw = dict(_kw(case), shift=case.shift[-1], scale=case.scale[-1])
    _, _, alone = sd.conditional_box_probabilities(case.L, case.lo[-1], case.hi[-1], case.n, case.seeds, case.dof,
                                                   return_integrand=True, return_mixing=True, **kw)
    assert _same(alone, s) and _same(_draws(case)[1], s)
    if case.M <= 3:                                                                         # another mixing stream: other scales
        other = sd.conditional_box_probabilities(case.L, case.lo, case.hi, case.n, case.seeds, case.dof, mix_stream=9,
                                                 return_mixing=True, **_kw(case))[1]
        p0 = tb.mixing_points(case.seeds[0], case.first, case.n, case.qmc, stream=9)
        assert _same(other[0], sd.conditional_mixing_scale(p0, case.dof_mix)) and not _same(other, s)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_diagonal_identity(hip, case):
    """f[r, b, j] == f[j-th box, point j] of the Gaussian entry on the n boxes ((lo_b - mu_b) / (r_b s_j), (hi_b - mu_b) / (r_b s_j))"""
    sd = _sd()
    res, f, s = _prob(case)
    streams = tb.chain_streams(case.M)
    for r, seed in enumerate(case.seeds):
        for b in range(case.B):
            lo_s, hi_s = ctc.scaled_limits(case.lo[b], case.hi[b], case.shift[b], case.scale[b], s[r])              # [n, M]
            _, fg = sd.copula_box_probabilities(case.L, lo_s, hi_s, case.n, [seed], streams=streams, first=case.first, qmc=case.qmc,
                                                return_integrand=True)
            assert _same(f[r, b], np.diagonal(fg[0]))
            if b == 1:
                assert np.all(np.isinf(hi_s))                                               # infinite limits stay infinite
    assert np.all(np.isfinite(f) & (f >= 0) & (f <= 1))
    if case.B == 4:
        assert np.all(f[:, 3] == 0.0) and np.all(res.replicates[:, 3] == 0.0)               # the empty component: exactly 0
        assert np.any(np.isinf(case.hi[1])) and np.any(f[:, 1] > 0)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_reduction_to_the_t_entries(hip, case):
    """zero shift (NULL), unit scale (NULL) and dof_mix = dof: the bits of copula_box_probabilities / copula_box_draws(dof=...)"""
    sd = _sd()
    kw = dict(first=case.first, qmc=case.qmc, return_mixing=True)
    want = sd.copula_box_probabilities(case.L, case.lo, case.hi, case.n, case.seeds, dof=case.dof, return_integrand=True, **kw)
    wantd = sd.copula_box_draws(case.L, case.lo, case.hi, case.n, case.seeds, dof=case.dof, **kw)
    for more in (dict(), dict(dof_mix=case.dof, scale=np.ones(case.B))):
        got = sd.conditional_box_probabilities(case.L, case.lo, case.hi, case.n, case.seeds, case.dof, return_integrand=True, **kw, **more)
        assert _same(got[0].replicates, want[0].replicates) and _same(got[1], want[1]) and _same(got[2], want[2])
        gotd = sd.conditional_box_draws(case.L, case.lo, case.hi, case.n, case.seeds, case.dof, **kw, **more)
        assert _same(gotd[0].z, wantd[0].z) and _same(gotd[0].u, wantd[0].u) and _same(gotd[0].weights, wantd[0].weights)
        assert _same(gotd[0].prob.replicates, wantd[0].prob.replicates) and _same(gotd[1], wantd[1])


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_mean_is_the_tree_of_the_integrand(hip, case):
    res, f, _ = _prob(case)
    # M = 1 uses its mixing point: the tree, as for every other M
    want = np.array([[bc.tree_mean(f[r, b], case.first) for b in range(case.B)] for r in range(len(case.seeds))])
    assert _same(res.replicates, want)
    assert _same(res.prob, res.replicates.mean(axis=0)) and res.n == case.n and np.array_equal(res.seeds, case.seeds)
    assert _same(_sd().conditional_box_probabilities(case.L, case.lo, case.hi, case.n, case.seeds, case.dof,
                                                     **_kw(case)).replicates, want)          # without f_out and s_out


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
    assert np.all(np.broadcast_to(box.z == hi, box.z.shape)[~inside])                      # an empty component gives hi
    finite = np.isfinite(box.z)
    # the map takes the copula's dof, not dof_mix (every case has dof_mix != dof)
    u = np.minimum(np.maximum(sd.student_t_cdf(np.where(finite, box.z, 0.0), case.dof), CLAMP_LO), CLAMP_HI)
    assert _same(box.u[finite], u[finite])
    assert case.dof_mix != case.dof
    if case.dof_mix <= 64:
        wrong = np.minimum(np.maximum(sd.student_t_cdf(np.where(finite, box.z, 0.0), case.dof_mix), CLAMP_LO), CLAMP_HI)
        assert not _same(box.u[finite], wrong[finite])
    # the chain's normals are those of the Gaussian draws entry on the scaled boxes; one rounded product, one rounded sum, clipped
    streams = tb.chain_streams(M, draws=True)
    for r, seed in enumerate(case.seeds):
        for b in range(B):
            lo_s, hi_s = ctc.scaled_limits(case.lo[b], case.hi[b], case.shift[b], case.scale[b], s[r])
            g = sd.copula_box_draws(case.L, lo_s, hi_s, n, [seed], streams=streams, first=case.first, qmc=case.qmc)
            zn = g.z[0][np.arange(n), :, np.arange(n)].T                                                        # [M, n]: box j, point j
            c = np.float64(case.scale[b]) * s[r]
            want = np.minimum(np.maximum(case.shift[b][:, None] + zn * c[None, :], case.lo[b][:, None]), case.hi[b][:, None])
            assert _same(box.z[r, b], want)
            assert _same(box.weights[r, b], np.diagonal(g.weights[0]))


def test_independence_and_repeatability(hip, monkeypatch):
    import torch
    sd = _sd()
    for case in (CASES[2], CASES[6]):                                                       # Philox n = 200 at 37, Sobol' n = 256
        res, f, s = _prob(case)
        box, _ = _draws(case)
        kw = dict(first=case.first, qmc=case.qmc, dof_mix=case.dof_mix)

        def prob(lo=case.lo, hi=case.hi, shift=case.shift, scale=case.scale, n=case.n, seeds=case.seeds, **more):
            args = dict(kw, return_integrand=True, return_mixing=True)
            args.update(more)
            return sd.conditional_box_probabilities(case.L, lo, hi, n, seeds, case.dof, shift=shift, scale=scale, **args)

        def draws(lo=case.lo, hi=case.hi, shift=case.shift, scale=case.scale, n=case.n, seeds=case.seeds, **more):
            args = dict(kw, return_mixing=True)
            args.update(more)
            return sd.conditional_box_draws(case.L, lo, hi, n, seeds, case.dof, shift=shift, scale=scale, **args)

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
        # calls split over boxes (a box alone, and in another position), seeds and point ranges
        for b in range(case.B):
            one = dict(lo=case.lo[b], hi=case.hi[b], shift=case.shift[b], scale=case.scale[b])
            pb, db = prob(**one), draws(**one)
            check(pb, db, boxes=slice(b, b + 1))
            assert _same(pb[0].replicates[:, 0], res.replicates[:, b])
        back = slice(None, None, -1)
        pr = prob(lo=case.lo[back], hi=case.hi[back], shift=case.shift[back], scale=case.scale[back])
        assert _same(pr[1][:, back], f) and _same(pr[0].replicates[:, back], res.replicates)
        front = (99,) + case.seeds
        pf, df = prob(seeds=front), draws(seeds=front)
        check((pf[0], pf[1][1:], pf[2][1:]), (sd.BoxDraws(df[0].z[1:], df[0].u[1:], df[0].weights[1:], None), df[1][1:]))
        assert _same(pf[0].replicates[1:], res.replicates)
        half = case.n // 2 - 3
        for c0, c1 in ((0, half), (half, case.n)):
            pr, dr = prob(n=c1 - c0, first=case.first + c0), draws(n=c1 - c0, first=case.first + c0)
            check(pr, dr, cols=slice(c0, c1))


# ---- the errors of the entries ----------------------------------------------------------------------------------------------------
def _raw(hip, entry, M=2, L=None, lo=(-1.0, -1.0), hi=(1.0, 1.0), dof=3.0, dof_mix=4.0, shift=(0.1, -0.2), scale=(1.5,), seeds=(0,),
         streams=None, mix=7, first=0, n=64, flags=8, kind=0):
    L = np.ascontiguousarray(np.eye(2) if L is None else L, dtype=np.float64)
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    shift = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
    scale = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
    B = lo.size // max(M, 1)
    seeds = np.asarray(seeds, dtype=np.uint64)
    streams = None if streams is None else np.asarray(streams, dtype=np.uint32)
    mean = np.full((seeds.size, B), -7.0)
    size = max(seeds.size * B * max(n, 0), 1)
    f, z = np.empty(size), np.empty(size * max(M, 1))
    if entry == "mlmc_copula_box_prob_tc_batch":
        rc = hip.lib().mlmc_copula_box_prob_tc_batch(M, hip.ptr(L), B, hip.ptr(lo), hip.ptr(hi), dof, dof_mix, hip.ptr(shift), hip.ptr(scale),
                                                     seeds.size, hip.ptr(seeds), hip.ptr(streams), mix, first, n, flags, hip.ptr(mean),
                                                     None, None, kind)
    else:
        rc = hip.lib().mlmc_copula_box_draws_tc_batch(M, hip.ptr(L), B, hip.ptr(lo), hip.ptr(hi), dof, dof_mix, hip.ptr(shift),
                                                      hip.ptr(scale), seeds.size, hip.ptr(seeds), hip.ptr(streams), mix, first, n, flags,
                                                      hip.ptr(mean), hip.ptr(f), hip.ptr(z), None, None, kind)
    return rc, mean, hip.lib().mlmc_last_error().decode()


@pytest.mark.parametrize("entry", ["mlmc_copula_box_prob_tc_batch", "mlmc_copula_box_draws_tc_batch"])
def test_errors_of_the_entry(hip, entry):
    rc, mean, _ = _raw(hip, entry)
    assert rc == 0 and 0 < mean[0, 0] < 1
    draws = entry.endswith("draws_tc_batch")
    for kw, match in ((dict(dof=0.5), "dof must lie in"),
                      (dict(dof=64.5), "dof must lie in"),
                      (dict(dof=np.nan), "dof must lie in"),
                      (dict(dof_mix=0.5), "dof_mix must lie in"),
                      (dict(dof_mix=192.5), "dof_mix must lie in"),
                      (dict(dof_mix=np.nan), "dof_mix must lie in"),
                      (dict(scale=[0.0]), "box 0: the scale must be finite and positive"),
                      (dict(scale=[-1.0]), "scale"),
                      (dict(scale=[np.inf]), "scale"),
                      (dict(scale=[np.nan]), "scale"),
                      (dict(shift=[0.0, np.inf]), "box 0, component 1: the shift is not finite"),
                      (dict(shift=[np.nan, 0.0]), "shift"),
                      (dict(mix=0), "mix_stream equals the stream of coordinate 0"),
                      (dict(streams=[5, 7] if draws else [7]), "mix_stream equals the stream of coordinate {}".format(1 if draws else 0)),
                      (dict(mix=1024), "mix_stream 1024 is not a Sobol' dimension"),
                      (dict(M=0), "M < 1"),
                      (dict(L=np.diag([1.0, 0.0])), "row 1"),
                      (dict(lo=[-1.0, np.nan]), "box 0, component 1"),
                      (dict(first=2 ** 52 - 63), "2\\^52"),
                      (dict(n=0), "n < 1"),
                      (dict(seeds=[]), "R < 1"),
                      (dict(flags=1), "ANTITHETIC"),
                      (dict(kind=5), "mem_kind")):
        rc, mean, msg = _raw(hip, entry, **kw)
        assert rc != 0 and re.search(match, msg) and msg.startswith(entry + ":"), (kw, msg)
        assert np.all(mean == -7.0)
    # the ends of the intervals, NULL shift and scale, the last point of the sequence
    assert _raw(hip, entry, dof=64.0, dof_mix=192.0)[0] == 0 and _raw(hip, entry, dof=1.0, dof_mix=1.0)[0] == 0
    assert _raw(hip, entry, shift=None, scale=None)[0] == 0
    assert _raw(hip, entry, first=2 ** 52 - 64)[0] == 0
