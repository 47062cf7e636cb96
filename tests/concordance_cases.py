"""The concordance counts of include/mlmc_hip.h (mlmc_concordance_counts) restated in NumPy, the level statistics that follow from
them, and the two copula cases shared by tests/test_concordance_cpu.py, tests/test_gpu_concordance.py and
tests/test_gpu_concordance_api.py.  Nothing here touches the device.

The twin is built from boolean arrays and np.count_nonzero: it shares no code shape with the kernel (no bit words, no popcount).

The copula cases: M = 3, latent correlations CORR, two levels of N_LEVEL samples each.  Level 0 is fine-only; the coarse values of
level 1 come from normals correlated COARSE_RHO with the fine ones (the same latent correlation between the components).  The
Gaussian case maps the normals through Phi; the Student-t case divides fine and coarse by the same sqrt(chi2_3 / 3) and maps through
the t_3 CDF: a copula with the same correlations and upper and lower tail dependence.  The model is the bivariate normal orthant
at CORR, which is the copula's own correlation in the Gaussian case.

Observed on the twin alone (N_LEVEL = 2^18, SEED below; tests/test_concordance_cpu.py prints them), pairs (0, 1), (0, 2), (1, 2):
    Gaussian, p = 0.9 :  z = Z_GAUSS[0]     p = 0.95:  z = Z_GAUSS[1]        bound: |z| < Z_BOUND = 5 (the score-correlation tests')
    Student-t, p = 0.9:  z = Z_T[0]                                          bound: z > Z_T_BOUND = 8
z grows like sqrt(n): 16384 samples per level gave 3.5 / 5.4 / 6.6 for the t case, so 2^18 puts it at 4 x that."""
import numpy as np
from scipy import special, stats

CORR = np.array([[1.0, 0.6, 0.5], [0.6, 1.0, 0.3], [0.5, 0.3, 1.0]])
COARSE_RHO = 0.98
PROBS = (0.9, 0.95)
N_LEVEL = 2 ** 18
SEED = 20261020
T_DOF = 3
Z_BOUND = 5.0
Z_T_BOUND = 8.0
# recorded from the twin (test_concordance_cpu.py::test_copula_cases_on_the_twin asserts them to 3 digits)
Z_GAUSS = ((-1.1256, 0.0292, 0.0486), (-0.6091, 0.5525, 0.3519))
Z_T = ((15.4792, 18.0895, 23.0537), (17.4393, 21.9125, 24.5566))


def twin_counts(fine, coarse, lower, upper):
    """-> pair [G, 3, M, M], all [G, 3], kept (int64): the definition of the header, one boolean array at a time"""
    fine = np.asarray(fine, dtype=np.float64)
    M, n = fine.shape
    lower = np.broadcast_to(np.atleast_2d(np.asarray(lower, dtype=np.float64)), (np.atleast_2d(lower).shape[0], M))
    upper = np.broadcast_to(np.atleast_2d(np.asarray(upper, dtype=np.float64)), (lower.shape[0], M))
    G = lower.shape[0]
    keep = ~np.isnan(fine).any(axis=0)
    if coarse is not None:
        coarse = np.asarray(coarse, dtype=np.float64)
        keep &= ~np.isnan(coarse).any(axis=0)
    pair = np.zeros((G, 3, M, M), dtype=np.int64)
    all_ = np.zeros((G, 3), dtype=np.int64)
    for g in range(G):
        with np.errstate(invalid="ignore"):
            ef = (lower[g][:, None] < fine) & (fine < upper[g][:, None]) & keep[None, :]
            ec = np.zeros_like(ef) if coarse is None else (lower[g][:, None] < coarse) & (coarse < upper[g][:, None]) & keep[None, :]
        for a in range(M):
            jf = ef[a][None, :] & ef
            jc = ec[a][None, :] & ec
            pair[g, 0, a] = np.count_nonzero(jf, axis=1)
            pair[g, 1, a] = np.count_nonzero(jc, axis=1)
            pair[g, 2, a] = np.count_nonzero(jf != jc, axis=1)
        af = np.all(ef, axis=0) & keep if M else keep.copy()
        ac = np.all(ec, axis=0) & keep if (M and coarse is not None) else np.zeros(n, dtype=bool)
        all_[g] = np.count_nonzero(af), np.count_nonzero(ac), np.count_nonzero(af != ac)
    return pair, all_, np.int64(np.count_nonzero(keep))


def twin_level_statistics(n, counts):
    """counts [L, ..., 3, ...] with the axis of 3 at position 2 (pair [L, G, 3, M, M] or all [L, G, 3]) and n [L]
    -> l_means, l_vars [L, G, ...], prob, var [G, ...]: mean_l = S / n_l, var_l = (Q - S^2 / n_l) / (n_l - 1), inf for n_l <= 1"""
    counts = np.asarray(counts)
    l_means, l_vars = [], []
    for l, nl in enumerate(np.asarray(n)):
        S = (counts[l, :, 0] - counts[l, :, 1]).astype(np.float64)
        Q = counts[l, :, 2].astype(np.float64)
        with np.errstate(all="ignore"):
            l_means.append(S / float(nl))
            l_vars.append((Q - S * S / float(nl)) / (float(nl) - 1.0) if nl > 1 else np.full(S.shape, np.inf))
    l_means, l_vars = np.array(l_means), np.array(l_vars)
    with np.errstate(all="ignore"):
        var = sum(v / float(nl) for v, nl in zip(l_vars, n))
    return l_means, l_vars, l_means.sum(axis=0), var


def copula_levels(kind, n=N_LEVEL, seed=SEED):
    """[(u_fine [3, n], None), (u_fine, u_coarse)]: the uniforms of the two levels of the 'gauss' or 't' case, inside (0, 1)"""
    rng = np.random.default_rng([seed, 0 if kind == "gauss" else 1])
    F = np.linalg.cholesky(CORR)
    levels = []
    for l in range(2):
        zf = F @ rng.standard_normal((3, n))
        zc = None if l == 0 else COARSE_RHO * zf + np.sqrt(1.0 - COARSE_RHO ** 2) * (F @ rng.standard_normal((3, n)))
        if kind == "gauss":
            to_u = special.ndtr
        else:
            scale = np.sqrt(rng.chisquare(T_DOF, size=n) / T_DOF)

            def to_u(z, scale=scale):
                return stats.t.cdf(z / scale, T_DOF)
        uf = np.clip(to_u(zf), 2.0 ** -53, 1.0 - 2.0 ** -53)
        uc = None if zc is None else np.clip(to_u(zc), 2.0 ** -53, 1.0 - 2.0 ** -53)
        levels.append((uf, uc))
    return levels


def upper_events(probs, M):
    """lower, upper [G, M] of the events u > p"""
    p = np.asarray(probs, dtype=np.float64)
    return p[:, None] * np.ones((p.size, M)), np.full((p.size, M), np.inf)


def model_orthant(probs, corr):
    """[G, M, M]: the bivariate normal orthant at the scores of the levels and `corr`"""
    from mlmc_amd.tool import simple_distribution as sd
    h = special.ndtri(np.asarray(probs, dtype=np.float64))[:, None, None]
    return sd.bivariate_orthant(h, h, np.asarray(corr)[None])


def z_scores(prob, var, model):
    with np.errstate(all="ignore"):
        return (prob - model) / np.sqrt(var)


def twin_tail_z(levels, probs=PROBS, corr=CORR):
    """the twin end to end on uniforms: -> prob, var, z [G, M, M]"""
    M = levels[0][0].shape[0]
    lower, upper = upper_events(probs, M)
    counts = [twin_counts(f, c, lower, upper) for f, c in levels]
    n = np.array([c[2] for c in counts])
    _, _, prob, var = twin_level_statistics(n, np.array([c[0] for c in counts]))
    return prob, var, z_scores(prob, var, model_orthant(probs, corr))


def off_diagonal(z):
    """[G, M (M - 1) / 2]: the pairs a < b in row order"""
    iu = np.triu_indices(z.shape[-1], 1)
    return z[:, iu[0], iu[1]]
