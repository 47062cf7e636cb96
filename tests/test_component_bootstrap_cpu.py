"""CPU tests of the per-component bootstrap: the two new C-ABI entries in header, binding and library, the host helper of the quantile
bands, and the argument checks of est_bootstrap_components / bootstrap_component_quantiles that come before any device call."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"mlmc_bootstrap_create_multi": 6, "mlmc_bootstrap_finalize_multi": 4}


def test_symbols_in_header_version_comment_binding_and_library():
    from mlmc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mlmc_hip.h")).read()
    version_comment = re.search(r"#define MLMC_ABI_VERSION \d+\s*/\*(.*?)\*/", hdr, flags=re.S).group(1)
    lib = _lib.load()
    for name, n_args in ENTRIES.items():
        assert re.search(r"\bint {}\s*\(".format(name), hdr), name
        assert re.search(r"\b{}\b".format(name), version_comment), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
        assert hasattr(lib, name), name


def test_abi_version_stays_8():
    from mlmc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mlmc_hip.h")).read()
    assert int(re.search(r"#define MLMC_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert _lib.ABI_VERSION == 8 and _lib.load().mlmc_abi_version() == 8


def test_entry_points_exist():
    from mlmc_amd import engine
    from mlmc_amd import estimator
    from mlmc_amd.quantity import quantity_estimate as qe
    assert issubclass(engine.ComponentBootstrapAccumulator, engine.BootstrapAccumulator)
    assert callable(qe.bootstrap_component_moments)
    assert callable(estimator.Estimate.est_bootstrap_components) and callable(estimator.Estimate.bootstrap_component_quantiles)
    assert estimator.ComponentBootstrapReplicates._fields == ("n_samples", "l_means", "l_vars", "mean", "var", "seed")
    assert estimator.QuantileBands._fields == ("q", "lo", "hi", "replicates", "success", "n_ok", "seed")


# ---- quantile_bands ------------------------------------------------------------------------------------------------------------------
def _replicates(B=41, M=3, P=4, seed=2):
    rng = np.random.default_rng(seed)
    rep = np.sort(rng.normal(size=(B, M, P)), axis=2)
    success = rng.random(size=(B, M)) < 0.8
    success[0] = True
    return rep, success


@pytest.mark.parametrize("level", [0.9, 0.5, 0.99])
def test_quantile_bands_equal_percentiles_of_the_successful_rows(level):
    from mlmc_amd.estimator import quantile_bands
    rep, success = _replicates()
    lo, hi = quantile_bands(rep, success, level)
    assert lo.shape == hi.shape == (3, 4)
    for m in range(3):
        rows = rep[success[:, m], m]
        assert np.array_equal(lo[m], np.percentile(rows, 100 * (1 - level) / 2, axis=0))
        assert np.array_equal(hi[m], np.percentile(rows, 100 * (1 + level) / 2, axis=0))
    assert np.all(lo <= hi)


def test_quantile_bands_exclude_failed_rows():
    from mlmc_amd.estimator import quantile_bands
    rep, success = _replicates()
    success[:] = True
    success[7, 1] = False
    spoiled = rep.copy()
    spoiled[7, 1] = 1e30                                   # the failed row's values must not matter
    a, b = quantile_bands(rep, success, 0.9), quantile_bands(spoiled, success, 0.9)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    success[7, 1] = True
    c = quantile_bands(spoiled, success, 0.9)
    assert not np.array_equal(a[1][1], c[1][1]) and np.array_equal(a[1][[0, 2]], c[1][[0, 2]])


def test_quantile_bands_nan_without_a_success():
    from mlmc_amd.estimator import quantile_bands
    rep, success = _replicates()
    success[:, 2] = False
    lo, hi = quantile_bands(rep, success, 0.9)
    assert np.all(np.isnan(lo[2])) and np.all(np.isnan(hi[2]))
    assert np.all(np.isfinite(lo[:2])) and np.all(np.isfinite(hi[:2]))
    # a single successful row: both ends are that row
    success[5, 2] = True
    lo, hi = quantile_bands(rep, success, 0.9)
    assert np.array_equal(lo[2], rep[5, 2]) and np.array_equal(hi[2], rep[5, 2])


@pytest.mark.parametrize("level", [0.0, 1.0, -0.1, 1.5, float("nan"), True, "0.9"])
def test_quantile_bands_level_outside_the_open_interval(level):
    from mlmc_amd.estimator import quantile_bands
    rep, success = _replicates()
    with pytest.raises(ValueError, match="level"):
        quantile_bands(rep, success, level)


def test_quantile_bands_shapes():
    from mlmc_amd.estimator import quantile_bands
    rep, success = _replicates()
    with pytest.raises(ValueError, match="success"):
        quantile_bands(rep, success[:, :2], 0.9)


# ---- argument checks before the device -------------------------------------------------------------------------------------------------
def _estimate(M=3):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    from mlmc_amd.sample_storage import Memory
    spec = [QuantitySpec(name="q", unit="m", shape=(M, 1), times=[1], locations=['0'])]
    st = Memory()
    st.save_global_data(result_format=spec, level_parameters=[[0.5], [0.1]])
    rng = np.random.default_rng(5)
    st.set_level_samples(0, rng.normal(size=(50, M)), None)
    st.set_level_samples(1, rng.normal(size=(20, M)), rng.normal(size=(20, M)))
    q = make_root_quantity(st, spec)['q'][1]['0']
    return Estimate(q, st, Legendre(4, (-3.0, 3.0)))


def _no_device(monkeypatch):
    from mlmc_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(_lib, "lib", no_device)
    monkeypatch.setattr(_lib, "init", no_device)


def _bad_fns():
    from mlmc_amd import Legendre, Monomial
    from mlmc_amd.moments import Spline, TransformedMoments
    leg = lambda R=4: Legendre(R, (-3.0, 3.0))
    return {
        "too_few": ([leg(), leg()], "2 moments objects for 3 components"),
        "mixed_sizes": ([leg(), leg(5), leg()], "same size"),
        "spline": ([Spline(6, (-3.0, 3.0))] * 3, "scalar_component"),
        "transformed": ([TransformedMoments(leg(), np.eye(3, 4))] * 3, "scalar_component"),
        "mixed_families": ([leg(), Monomial(4, (-3.0, 3.0)), leg()], "scalar_component"),
    }


@pytest.mark.parametrize("case", list(_bad_fns()))
def test_components_moments_fns_errors_before_the_device(monkeypatch, case):
    fns, match = _bad_fns()[case]
    est = _estimate()
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match=match):
        est.est_bootstrap_components(10, moments_fns=fns, seed=1)


@pytest.mark.parametrize("kwargs,match", [
    (dict(n_subsamples=0), "n_subsamples"),
    (dict(n_subsamples=2.5), "n_subsamples"),
    (dict(n_subsamples=True), "n_subsamples"),
    (dict(sample_vector=[10, 21]), "0 .. n_collected"),
    (dict(sample_vector=[-1, 5]), "0 .. n_collected"),
    (dict(sample_vector=[10.5, 5]), "integer"),
    (dict(sample_vector=[10]), "integer"),
    (dict(seed=-3), "seed"),
    (dict(seed=2 ** 64), "seed"),
    (dict(seed=1.5), "seed"),
])
def test_components_argument_errors_before_the_device(monkeypatch, kwargs, match):
    est = _estimate()
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match="est_bootstrap_components: .*" + match):
        est.est_bootstrap_components(**kwargs)


@pytest.mark.parametrize("kwargs,match", [
    (dict(probs=[0.05, 0.5], level=0.0), "level"),
    (dict(probs=[0.05, 0.5], level=1.0), "level"),
    (dict(probs=[0.05, 0.5], level=1.3), "level"),
    (dict(probs=[0.05, 0.5], level=float("nan")), "level"),
    (dict(probs=[0.05, float("nan")]), "probs"),
    (dict(probs=[0.05, 1.5]), "probs"),
    (dict(probs=[]), "probs"),
    (dict(probs=[0.5], n_subsamples=0), "n_subsamples"),
    (dict(probs=[0.5], seed=-1), "seed"),
])
def test_quantile_bands_argument_errors_before_the_device(monkeypatch, kwargs, match):
    est = _estimate()
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match="bootstrap_component_quantiles: .*" + match):
        est.bootstrap_component_quantiles(**kwargs)
