"""CPU tests of the normal-score correlation: the inputs of tests/test_gpu_normal_scores.py pass by the reference alone (closed-form
quantiles, SciPy's ndtri), the semantics of mlmc_density_scores_batch restated in NumPy (tests/score_cases.py), and the argument
checks of the Python layers that need no device."""
import numpy as np
import pytest
from scipy import special

from tests import score_cases as sk


def _sd():
    from mlmc_amd.tool import simple_distribution as sd
    return sd


@pytest.mark.parametrize("first", sk.FIRSTS)
def test_copula_case_by_the_reference(first):
    """closed-form draws of the copula case: the correlations of the normal scores ndtri(F(x)) lie within 5 standard errors
    (1 - rho^2) / sqrt(n) of the latent ones, the Pearson correlation of the (5, -5) pair is more than 20 away from 0.8"""
    F, info = _sd().correlation_factor(sk.CORR)
    assert not info.repaired
    x, y = sk.copula_case(first, F)
    assert x.shape == (3, sk.N_COPULA)
    for row, dom in zip(x, sk.DOMAINS):
        assert np.all((row > dom[0]) & (row < dom[1]))
    z = np.array([sk.twin_scores(lambda v, r=r, d=d: sk.closed_cdf(r, d, v), d, row)[0] for r, d, row in zip(sk.RATES, sk.DOMAINS, x)])
    assert np.all(np.isfinite(z)) and np.max(np.abs(z - y)) <= 1e-9                    # the round trip through Q and F
    score_err = sk.standard_errors(z, sk.CORR)
    pearson_err = sk.standard_errors(x, sk.CORR)
    print(f"\nfirst = {first}: scores {score_err.max():.3g} standard errors; Pearson of the (5, -5) pair {np.corrcoef(x)[0, 1]:.4f}, "
          f"{pearson_err[0]:.3g} standard errors from 0.8")
    assert score_err.max() <= 5.0
    assert pearson_err[0] > 20.0


def test_closed_forms():
    """F and Q of the truncated exponentials are inverse to each other, F is the integral of exp(-r t), the multipliers give unit mass"""
    p = np.linspace(0.001, 0.999, 97)
    t = np.linspace(-1.0, 1.0, 200001)
    for rate, dom in zip(sk.RATES, sk.DOMAINS):
        x = sk.closed_quantile(rate, dom, p)
        assert np.all(np.diff(x) > 0) and np.all((x > dom[0]) & (x < dom[1]))
        # a few roundings of F itself, and the rounding of x (4 spacings) times the largest density, below max(|r|, 1) 2 / (b - a)
        slack = 8 * sk.U + 4 * np.spacing(max(abs(dom[0]), abs(dom[1]))) * max(abs(rate), 1.0) * 2.0 / (dom[1] - dom[0]) * 1.01
        assert np.max(np.abs(sk.closed_cdf(rate, dom, x) - p)) <= slack
        lam = sk.multipliers(rate)
        rho = np.exp(-lam[0] - lam[1] * t)
        cum = np.concatenate([[0.0], np.cumsum(0.5 * (rho[1:] + rho[:-1]) * np.diff(t))])
        assert abs(cum[-1] - 1.0) <= 1e-8
        xt = dom[0] + 0.5 * (dom[1] - dom[0]) * (t + 1.0)
        assert np.max(np.abs(sk.closed_cdf(rate, dom, xt) - cum)) <= 1e-8


def test_semantics_of_the_twin():
    """NaN, values outside the domain and the end points themselves give NaN; exactly the strictly-inside values are finite; the
    clamp: u below 2^-53 gives ndtri(2^-53), u = 1 gives ndtri(1 - 2^-53)"""
    dom = (0.5, 4.5)
    a, b = dom
    x = np.array([np.nan, -np.inf, np.inf, a, b, np.nextafter(a, b), np.nextafter(a, -np.inf), np.nextafter(b, a), np.nextafter(b, np.inf),
                  1e300, 2.0])
    inside = np.array([False, False, False, False, False, True, False, True, False, False, True])
    for rate in sk.RATES:
        z, u = sk.twin_scores(lambda v: sk.closed_cdf(rate, dom, v), dom, x)
        assert np.array_equal(np.isfinite(z), inside) and np.array_equal(np.isfinite(u), inside)
        assert np.all(np.isnan(z[~inside])) and np.all(np.isnan(u[~inside]))
    z, u = sk.twin_scores(lambda v: np.where(v < 1.0, 0.0, np.where(v > 4.0, 1.0, 0.25)), dom, np.array([0.75, 4.25, 2.0]))
    assert np.array_equal(u, [0.0, 1.0, 0.25])
    assert z[0] == special.ndtri(sk.U_LO) and z[1] == special.ndtri(sk.U_HI) and z[2] == special.ndtri(0.25)
    assert -8.3 < z[0] < -8.2 and 8.2 < z[1] < 8.3


class _Rule:
    def __init__(self, n_intervals=64, gauss_degree=21):
        self.n_intervals, self._gauss_degree = n_intervals, gauss_degree


def test_normal_scores_argument_errors():
    """checked before anything touches the device"""
    sd = _sd()
    three = [_Rule()] * 3
    with pytest.raises(ValueError, match="no distributions"):
        sd.normal_scores([], np.zeros((0, 4)))
    with pytest.raises(ValueError, match="normal_scores: every distribution must use the same quadrature"):
        sd.normal_scores([_Rule(), _Rule(200), _Rule()], np.zeros((3, 4)))
    with pytest.raises(ValueError, match="normal_scores: every distribution must use the same quadrature"):
        sd.normal_scores([_Rule(), _Rule(64, 10)], np.zeros((2, 4)))
    with pytest.raises(ValueError, match=r"fine must be \[M, n\]"):
        sd.normal_scores(three, np.zeros((2, 4)))
    with pytest.raises(ValueError, match=r"fine must be \[M, n\]"):
        sd.normal_scores(three, np.zeros(4))
    with pytest.raises(ValueError, match=r"coarse must be \[M, n\]"):
        sd.normal_scores(three, np.zeros((3, 4)), np.zeros((4, 4)))
    with pytest.raises(ValueError, match="differ in shape"):
        sd.normal_scores(three, np.zeros((3, 4)), np.zeros((3, 5)))


def _estimate(M=3):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate

    class _Quantity:
        def size(self):
            return M
    return Estimate(_Quantity(), None, Legendre(3, (0.0, 1.0)))


def test_estimate_argument_errors():
    """corr strings other than "scores" and a list of densities of the wrong length are raised before a sample is read; the block
    constant of the score workspace"""
    from mlmc_amd.quantity import quantity_estimate as qe
    est = _estimate()
    for bad in ("pearson", "score", "Scores", ""):
        with pytest.raises(ValueError, match="corr must be None, 'scores' or a correlation matrix"):
            est.sample_joint(10, 1, corr=bad, densities=[(None, None, None, None)] * 3)
    with pytest.raises(ValueError, match="n must be"):
        est.sample_joint(-1, 1, corr="scores")
    with pytest.raises(ValueError, match="2 densities for 3 components"):
        est.estimate_score_correlation(densities=[(_Rule(),)] * 2)
    with pytest.raises(ValueError, match="densities must be the list"):
        est.estimate_score_correlation(densities="scores")
    assert qe.SCORE_BLOCK_BYTES == 64 << 20 and qe.score_block_columns(12) % 64 == 0
    assert 2 * 8 * 13 * qe.score_block_columns(12) <= qe.SCORE_BLOCK_BYTES < 2 * 8 * 13 * (qe.score_block_columns(12) + 64)
    assert qe.score_block_columns(1022) >= 64


def test_entry_is_declared():
    import os
    from mlmc_amd import _lib
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "include", "mlmc_hip.h")).read()
    name = "mlmc_density_scores_batch"
    assert name in text.split("#define MLMC_ABI_VERSION")[1].split("*/")[0]
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 19
    assert hasattr(_lib.load(), name)
