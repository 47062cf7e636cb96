"""CPU tests of the host side of the per-component moment estimates (Estimate.estimate_component_moments / _diff_vars /
_diff_vars_regression): argument checks before any device work, the regression of [L, M, R] level variances, the route
choice."""
import numpy as np
import pytest


def _storage(n_levels=3, n_comp=4):
    from mlmc_amd.sample_storage import Memory
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    rng = np.random.default_rng(11)
    spec = [QuantitySpec(name="q", unit="m", shape=(n_comp, 1), times=[1], locations=['0'])]
    st = Memory()
    steps = [0.5 * 0.3 ** l for l in range(n_levels)]
    st.save_global_data(result_format=spec, level_parameters=[[s] for s in steps])
    for l in range(n_levels):
        n = 40 - 5 * l
        st.set_level_samples(l, rng.normal(size=(n, n_comp)), None if l == 0 else rng.normal(size=(n, n_comp)))
    st.save_n_ops([(l, (10.0 * 4 ** l, 40 - 5 * l)) for l in range(n_levels)])
    return st, spec


def _estimate(n_levels=3, n_comp=4):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity.quantity import make_root_quantity
    st, spec = _storage(n_levels, n_comp)
    root = make_root_quantity(st, spec)['q'][1]['0']
    return Estimate(root, st, Legendre(5, (-2.0, 2.0))), st


def _no_device(monkeypatch):
    from mlmc_amd import _lib
    from mlmc_amd.quantity import quantity_estimate as qe

    def forbidden(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(qe, "component_level_sums", forbidden)
    monkeypatch.setattr(qe, "estimate_mean", forbidden)
    monkeypatch.setattr(_lib, "lib", forbidden)


@pytest.mark.parametrize("method", ["estimate_component_moments", "estimate_component_diff_vars",
                                    "estimate_component_diff_vars_regression"])
def test_wrong_moments_fns_raise_before_any_device_call(monkeypatch, method):
    from mlmc_amd import Legendre, Monomial
    est, _ = _estimate()
    _no_device(monkeypatch)
    call = getattr(est, method)
    args = ([100, 10, 3],) if method.endswith("regression") else ()
    with pytest.raises(ValueError, match="3 moments objects for 4 components"):
        call(*args, moments_fns=[Legendre(5, (-1.0, 1.0))] * 3)
    with pytest.raises(ValueError, match="same size"):
        call(*args, moments_fns=[Legendre(5, (-1.0, 1.0))] * 3 + [Monomial(6, (-1.0, 1.0))])
    with pytest.raises(ValueError, match="same size"):
        call(*args, moments_fns=[Legendre(5, (-1.0, 1.0)), Legendre(7, (-1.0, 1.0))] * 2)


def test_device_route_choice():
    from mlmc_amd import Legendre, Monomial, Fourier, Spline
    from mlmc_amd.moments import TransformedMoments
    from mlmc_amd.quantity import quantity_estimate as qe
    dom = (-1.0, 1.0)
    assert qe.component_device_route([Legendre(5, dom), Legendre(5, (0.5, 3.0), log=True)])
    assert qe.component_device_route([Monomial(4, dom)] * 3)
    assert qe.component_device_route([Fourier(7, dom)])
    assert not qe.component_device_route([Legendre(5, dom), Monomial(5, dom)])       # mixed families
    assert not qe.component_device_route([Spline(8, dom)] * 2)                        # splines take the loop
    assert not qe.component_device_route([Legendre(5, dom), Legendre(6, dom)])
    tm = TransformedMoments(Legendre(5, dom), np.eye(5))                            # transformed moments take the loop
    assert not qe.component_device_route([tm, tm])


@pytest.mark.parametrize("n_levels", [1, 2, 3, 5])
def test_component_regression_equals_the_regression_of_each_component(n_levels):
    est, st = _estimate(n_levels=n_levels)
    rng = np.random.default_rng(3)
    L, M, R = n_levels, 4, 5
    raw = np.exp(rng.normal(size=(L, M, R))) * (0.3 ** np.arange(L))[:, None, None]
    raw[:, :, 0] = 0.0                             # phi_0: zero level variances on every component
    raw[:, 2, 3] = 0.0                             # an all-zero column of one component
    raw[1:, 1, 4] = 1e-30                          # a column np.isclose takes for zero
    reg, n_ops = est.estimate_component_diff_vars_regression([100] * L, raw_vars=raw)
    assert reg.shape == (L, M, R)
    assert np.array_equal(n_ops, st.get_n_ops())
    assert est._n_created_samples == [100] * L
    sim_steps = np.squeeze(st.get_level_parameters())
    for m in range(M):
        ref = est._all_moments_variance_regression(raw[:, m, :], sim_steps)
        assert np.allclose(reg[:, m, :], ref, rtol=1e-12, atol=0), m
        assert np.array_equal(reg[0, m, :], raw[0, m, :])          # level 0 is never regressed
    assert np.array_equal(reg[:, :, 0], np.zeros((L, M)))
    assert np.array_equal(reg[:, 2, 3], np.zeros(L))
    if n_levels < 3:
        assert np.array_equal(reg, raw)
    # the sample allocation takes the [L, M * R] view
    from mlmc_amd.estimator import estimate_n_samples_for_target_variance
    n_est = estimate_n_samples_for_target_variance(1e-3, reg.reshape(L, -1), n_ops, n_levels=L)
    assert n_est.shape == (L,) and np.all(n_est >= 2)


def test_component_regression_rejects_a_flat_raw_vars():
    est, _ = _estimate()
    with pytest.raises(ValueError, match=r"\[L, M, R\]"):
        est.estimate_component_diff_vars_regression([100] * 3, raw_vars=np.ones((3, 20)))
