"""GPU tests of mlmc_student_t_quantile and mlmc_copula_log_density (include/mlmc_hip.h) against the references, twins and units
of tests/copula_lik_cases.py."""
import ctypes as C

import numpy as np
import pytest

from tests import copula_lik_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from mlmc_amd import _lib
    _lib.init(0)
    return _lib


def _sd():
    from mlmc_amd.tool import simple_distribution
    return simple_distribution


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ---- the quantile --------------------------------------------------------------------------------------------------------------

def test_quantile_against_mpmath(hip):
    sd = _sd()
    p = lc.p_arguments()
    worst = 0.0
    print("\n  nu | q units (at p)")
    for dof in lc.DOFS:
        y = sd.student_t_quantile(p, dof)
        units = np.array([lc.q_units(a, lc.mp_t_quantile(dof, v, a), v, dof) for a, v in zip(y, p)])
        i = int(np.argmax(units))
        print("{:4g} | {:8.2f} ({:12.5g})".format(dof, units[i], p[i]))
        worst = max(worst, float(units[i]))
        assert units[i] <= lc.Q_UNITS_GATE, (dof, p[i], units[i])
    print("largest: {:.2f} q_units, gate {:.2f}".format(worst, lc.Q_UNITS_GATE))


def test_quantile_symmetry_special_values_sizes_and_memory(hip):
    import torch
    sd = _sd()
    k = np.arange(1, 512) * 2.0 ** -10
    rng = np.random.default_rng(5)
    for dof in lc.DOFS:
        lower = sd.student_t_quantile(k, dof)
        assert _same(sd.student_t_quantile(1.0 - k, dof), -lower) and np.all(np.diff(lower) > 0.0) and np.all(lower < 0.0)
        special = sd.student_t_quantile(np.array([0.0, 1.0, 0.5, np.nan, -0.25, 1.0 + 2.0 ** -52, -0.0]), dof)
        assert special[0] == -np.inf and special[1] == np.inf and special[2] == 0.0 and not np.signbit(special[2])
        assert np.all(np.isnan(special[3:6])) and special[6] == -np.inf
        p = rng.random(257)
        full = sd.student_t_quantile(p, dof)
        for n in (1, 255, 256, 257):
            assert _same(sd.student_t_quantile(p[:n], dof), full[:n])
        on_device = sd.student_t_quantile(torch.from_numpy(p).cuda(), dof, device=True)
        assert on_device.is_cuda and _same(on_device.cpu().numpy(), full)
        back = sd.student_t_cdf(full, dof)
        assert np.max(np.abs(back - p) / np.minimum(p, 1.0 - p)) < 1e-12


# ---- the log density ------------------------------------------------------------------------------------------------------------

def _entry(hip, pr, models=None, coarse=True, cols=slice(None), pad=5, outputs=True, sums=True, device=False, u_fine=None):
    """one call of the C entry on the columns `cols` of a problem, rows pad columns longer than n: dict(y, ll_fine, ll_coarse, kept,
    sums); device: through device tensors"""
    import torch
    g = list(range(pr.G)) if models is None else list(models)
    G, M = len(g), pr.M
    A = np.ascontiguousarray(pr.A[g])
    logdet, dof = np.ascontiguousarray(pr.logdet[g]), np.ascontiguousarray(pr.dofs[g])

    def rows(u):
        u = u[:, :pr.n][:, cols]
        out = np.full((M, u.shape[1] + pad), 0.125)
        out[:, :u.shape[1]] = u
        return out
    uf = rows(pr.u_fine if u_fine is None else u_fine)
    uc = rows(pr.u_coarse) if (coarse and pr.u_coarse is not None) else None
    n, ld = uf.shape[1] - pad, uf.shape[1]
    ldo = n + 3
    y = np.full((G, M, ldo), 7.0) if outputs else None
    lf = np.full((G, ldo), 7.0) if outputs else None
    lcz = np.full((G, ldo), 7.0) if (outputs and uc is not None) else None
    kept = np.full(1, -1, dtype=np.int64) if sums else None
    out = np.full(3 * G + G * G, 7.0) if sums else None
    kind = hip.HOST
    arrays = [uf, uc, y, lf, lcz]
    if device:
        arrays = [None if a is None else torch.from_numpy(a).cuda() for a in arrays]
        torch.cuda.synchronize()
        kind = hip.DEVICE
    hip.check(hip.lib().mlmc_copula_log_density(M, G, hip.ptr(A), hip.ptr(logdet), hip.ptr(dof), hip.ptr(arrays[0]), hip.ptr(arrays[1]),
                                                n, ld, hip.ptr(arrays[2]), hip.ptr(arrays[3]), hip.ptr(arrays[4]), ldo, hip.ptr(kept),
                                                hip.ptr(out), kind))
    if device:
        arrays = [None if a is None else a.cpu().numpy() for a in arrays]
    y, lf, lcz = arrays[2:]
    if outputs:                                                     # nothing is written beyond column n
        assert np.all(y[:, :, n:] == 7.0) and np.all(lf[:, n:] == 7.0) and (lcz is None or np.all(lcz[:, n:] == 7.0))
    return dict(y=None if y is None else y[:, :, :n], ll_fine=None if lf is None else lf[:, :n],
                ll_coarse=None if lcz is None else lcz[:, :n], kept=None if kept is None else int(kept[0]), sums=out, n=n)


PROBLEMS = [lc.Problem(*shape) for shape in lc.SHAPES]
_WORST = {}


@pytest.mark.parametrize("pr", PROBLEMS, ids=repr)
def test_log_density(hip, pr):
    sd = _sd()
    res = _entry(hip, pr)
    keep = pr.keep
    assert res["kept"] == int(np.count_nonzero(keep))
    # dropped columns are NaN everywhere, kept ones finite
    for name in ("y", "ll_fine", "ll_coarse"):
        a = res[name]
        if a is None:
            assert name == "ll_coarse" and pr.u_coarse is None
            continue
        assert np.all(np.isnan(a[..., ~keep])) and np.all(np.isfinite(a[..., keep])), name
    # the scores of the coarse side: the entry on the coarse uniforms alone (a value depends on its column, model and side alone)
    sides = [(pr.u_fine, res["y"], res["ll_fine"])]
    if pr.u_coarse is not None:
        alone = _entry(hip, pr, coarse=False, u_fine=pr.u_coarse)
        both = keep & ~np.isnan(alone["ll_fine"][0])
        assert _same(alone["ll_fine"][:, both], res["ll_coarse"][:, both])
        sides.append((pr.u_coarse, alone["y"], alone["ll_fine"]))
    worst = 0.0
    for u, y, ll in sides:
        ok = ~np.isnan(ll[0])
        uc = lc.clamp(u[:, :pr.n][:, ok])
        for g, dof in enumerate(pr.dofs):
            if dof != np.inf:                                       # the t scores are those of the elementwise entry, bit for bit
                assert _same(y[g][:, ok], sd.student_t_quantile(uc, dof)), (g, dof)
            ref, scale = lc.long_double_log_density(pr.A[g], pr.logdet[g], dof, y[g][:, ok])
            units = lc.l_units(ll[g][ok], ref, scale)
            worst = max(worst, float(np.max(units)) if units.size else 0.0)
            assert np.all(units <= lc.L_UNITS_GATE), (g, dof, float(np.max(units)))
    _WORST[repr(pr)] = worst
    print("\n{}: at most {:.3f} l_units (gate {:.2f})".format(pr, worst, lc.L_UNITS_GATE))
    # the sums are the documented tree of the returned columns
    kept, want = lc.tree_sums(res["ll_fine"], res["ll_coarse"])
    assert kept == res["kept"] and _same(res["sums"], want)
    # without the optional arrays, and the sums alone
    bare = _entry(hip, pr, outputs=False)
    assert bare["kept"] == res["kept"] and _same(bare["sums"], res["sums"])
    assert _same(_entry(hip, pr, sums=False)["ll_fine"], res["ll_fine"])


def test_the_two_exact_zeros(hip):
    sd = _sd()
    rng = np.random.default_rng(9)
    u = rng.random((1, 130))
    u[0, :4] = (0.0, 1.0, lc.U, 1.0 - lc.U)
    dofs = (np.inf,) + tuple(lc.DOFS)
    out = sd.copula_log_density(u, np.ones((1, 1)), dofs)
    assert out.shape == (len(dofs), 130) and np.all(out == 0.0)
    for M in (2, 17, 128):
        u = rng.random((M, 70))
        assert np.all(sd.copula_log_density(u, np.eye(M), np.inf) == 0.0)


def test_independence_and_repeatability(hip, monkeypatch):
    for pr in (PROBLEMS[2], PROBLEMS[4]):                           # M = 3, G = 16, n = 64; M = 64, G = 3, n = 200
        res = _entry(hip, pr)
        keys = ("y", "ll_fine", "ll_coarse", "sums", "kept")

        def check(other, models=slice(None), cols=slice(None), sums=True, coarse=True):
            assert _same(other["y"], res["y"][models][:, :, cols]) and _same(other["ll_fine"], res["ll_fine"][models][:, cols])
            if coarse:
                assert _same(other["ll_coarse"], res["ll_coarse"][models][:, cols])
            if sums:
                assert _same(other["sums"], res["sums"]) and other["kept"] == res["kept"]

        check(_entry(hip, pr))                                      # a second run
        check(_entry(hip, pr, device=True))                         # device memory
        check(_entry(hip, pr, pad=64))                              # another row stride
        for pts in ("64", "130"):                                   # the launch split
            monkeypatch.setenv("MLMC_COPULA_LIK_BLOCK_POINTS", pts)
            check(_entry(hip, pr))
            check(_entry(hip, pr, device=True))
        monkeypatch.delenv("MLMC_COPULA_LIK_BLOCK_POINTS")
        # fewer columns, and columns at another position
        half = pr.n // 2 - 3
        for c0, c1 in ((0, half), (half, pr.n), (1, pr.n)):
            check(_entry(hip, pr, cols=slice(c0, c1)), cols=slice(c0, c1), sums=False)
        # fewer models, and the models in another order
        order = list(range(pr.G))[::-1]
        check(_entry(hip, pr, models=order), models=order, sums=False)
        check(_entry(hip, pr, models=[1]), models=[1], sums=False)
        # without the coarse side: the fine values of the columns that stay kept
        alone = _entry(hip, pr, coarse=False)
        both = pr.keep
        assert _same(alone["ll_fine"][:, both], res["ll_fine"][:, both]) and _same(alone["y"][:, :, both], res["y"][:, :, both])
        assert alone["ll_coarse"] is None and alone["kept"] >= res["kept"]
        G = pr.G
        # l^c = 0 without coarse: sum d = sum l^f, and the coarse sums are 0
        assert _same(alone["sums"][2 * G:3 * G], alone["sums"][:G]) and np.all(alone["sums"][G:2 * G] == 0.0)


def test_python_entry(hip):
    import torch
    sd = _sd()
    pr = PROBLEMS[3]                                                # M = 17, G = 2, n = 65, no coarse
    res = _entry(hip, pr)
    corr = [np.linalg.inv(a.T @ a) for a in pr.A]
    u = pr.u_fine[:, :pr.n]
    out = sd.copula_log_density(u, corr, pr.dofs, return_scores=True)
    assert out.coarse is None and out.fine.shape == (2, 65) and out.scores.shape == (2, 17, 65)
    # the factor is made anew from the correlation matrix: the values agree to rounding, the pattern of NaN exactly
    assert _same(np.isnan(out.fine), np.isnan(res["ll_fine"]))
    assert np.allclose(out.fine[:, pr.keep], res["ll_fine"][:, pr.keep], rtol=1e-9, atol=1e-9)
    assert _same(out.scores, res["y"])
    dev = sd.copula_log_density(torch.from_numpy(u).cuda(), corr, pr.dofs, device=True)
    assert dev.is_cuda and _same(dev.cpu().numpy(), out.fine)
    assert _same(sd.copula_log_density(u, corr, pr.dofs), out.fine)
    pair = sd.copula_log_density(u, corr[0], 3.0, u_coarse=u[:, ::-1].copy())
    assert pair.fine.shape == pair.coarse.shape == (1, 65) and pair.scores is None
    assert sd.copula_log_density(np.zeros((3, 0)), np.eye(3), (3.0, np.inf)).shape == (2, 0)


# ---- errors of the C entry: each is named, none touches the device ----------------------------------------------------------------

def test_entry_errors(hip):
    M, G, n = 3, 2, 10
    A = np.ascontiguousarray(np.stack([np.eye(M)] * G))
    base = dict(M=M, G=G, A=A, logdet=np.zeros(G), dof=np.array([3.0, np.inf]), u_fine=np.full((M, n), 0.5), u_coarse=None, n=n, ld=n,
                y_out=None, ll_fine=np.zeros((G, n)), ll_coarse=None, ldo=n, kept=np.zeros(1, dtype=np.int64),
                sums=np.zeros(3 * G + G * G), kind=hip.HOST)

    def call(**kw):
        a = dict(base)
        a.update(kw)
        return hip.lib().mlmc_copula_log_density(a["M"], a["G"], hip.ptr(a["A"]), hip.ptr(a["logdet"]), hip.ptr(a["dof"]),
                                                 hip.ptr(a["u_fine"]), hip.ptr(a["u_coarse"]), a["n"], a["ld"], hip.ptr(a["y_out"]),
                                                 hip.ptr(a["ll_fine"]), hip.ptr(a["ll_coarse"]), a["ldo"], hip.ptr(a["kept"]),
                                                 hip.ptr(a["sums"]), a["kind"])

    def bad_A(i, k, v, g=1):
        a = A.copy()
        a[g, i, k] = v
        return a
    cases = [
        (dict(M=0), "M < 1"), (dict(M=129), "M = 129 is above the cap 128"), (dict(G=0), "G < 1"), (dict(G=17), "G = 17 is above the cap 16"),
        (dict(A=None), "null model argument"), (dict(logdet=None), "null model argument"), (dict(dof=None), "null model argument"),
        (dict(n=-1), "n < 0"), (dict(ld=n - 1), "row stride ld = 9 is below n = 10"), (dict(kind=7), "bad mem_kind"),
        (dict(ldo=n - 1), "output stride ldo = 9 is below n = 10"), (dict(ll_coarse=np.zeros((G, n))), "ll_coarse without u_coarse"),
        (dict(ll_fine=None, kept=None, sums=None), "every output is null"),
        (dict(dof=np.array([3.0, 0.5])), "model 1: dof must lie in [1, 64] or be +inf"),
        (dict(dof=np.array([np.nan, 3.0])), "model 0: dof must lie in"), (dict(dof=np.array([3.0, -np.inf])), "model 1: dof must lie in"),
        (dict(logdet=np.array([0.0, np.nan])), "model 1: logdet is not finite"),
        (dict(A=bad_A(2, 2, 0.0)), "model 1, factor row 2: the diagonal entry must be finite and positive"),
        (dict(A=bad_A(1, 1, np.inf, g=0)), "model 0, factor row 1: the diagonal entry"),
        (dict(A=bad_A(2, 1, np.nan)), "model 1, factor row 2: entry 1 is not finite"),
        (dict(u_fine=None), "null u_fine"),
    ]
    for kw, message in cases:
        assert call(**kw) != 0, message
        assert message in hip.load().mlmc_last_error().decode(), (message, hip.load().mlmc_last_error().decode())
    # what lies above the diagonal is not read; n = 0 is a no-op that zeroes the sums
    assert call(A=bad_A(0, 2, np.nan)) == 0
    kept, sums = np.full(1, 5, dtype=np.int64), np.full(3 * G + G * G, 5.0)
    assert call(n=0, ld=0, ldo=0, u_fine=None, kept=kept, sums=sums) == 0 and kept[0] == 0 and np.all(sums == 0.0)
    for entry in ("mlmc_student_t_quantile",):
        for kw, message in ((dict(dof=0.5), "dof must lie in [1, 64]"), (dict(n=-1), "n < 0"), (dict(kind=5), "bad mem_kind"),
                            (dict(p=None), "null argument")):
            a = dict(dof=3.0, n=4, p=np.full(4, 0.5), out=np.zeros(4), kind=hip.HOST)
            a.update(kw)
            assert getattr(hip.lib(), entry)(C.c_double(a["dof"]), a["n"], hip.ptr(a["p"]), hip.ptr(a["out"]), a["kind"]) != 0
            assert message in hip.load().mlmc_last_error().decode(), message
