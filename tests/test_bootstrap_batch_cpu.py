"""CPU tests of the batched bootstrap: the new C-ABI entries in header, binding and library, the Python entry points, the argument
checks that come before any device call, and the host draws of the sub-sample sizes."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"mlmc_bootstrap_weights": 7, "mlmc_bootstrap_create": 5, "mlmc_bootstrap_destroy": 1, "mlmc_bootstrap_reset": 1,
           "mlmc_bootstrap_accum": 8, "mlmc_bootstrap_finalize": 4, "mlmc_bootstrap_kernel_time": 4}


def test_bootstrap_symbols_in_header_binding_and_library():
    from mlmc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mlmc_hip.h")).read()
    lib = _lib.load()
    for name, n_args in ENTRIES.items():
        assert re.search(r"\b{}\s*\(".format(name), hdr), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
        assert hasattr(lib, name), name


def test_abi_version_stays_8():
    from mlmc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mlmc_hip.h")).read()
    assert int(re.search(r"#define MLMC_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert _lib.ABI_VERSION == 8 and _lib.load().mlmc_abi_version() == 8


def test_bootstrap_entry_points_exist():
    from mlmc_amd import engine
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    assert callable(getattr(Estimate, "est_bootstrap_batch", None))
    assert callable(getattr(engine, "bootstrap_weights", None))
    assert isinstance(getattr(engine, "BootstrapAccumulator", None), type)
    assert callable(getattr(qe, "bootstrap_moments", None)) and callable(getattr(qe, "bootstrap_sizes", None))
    import inspect
    params = inspect.signature(Estimate.bs_target_var_n_estimated).parameters
    assert params["batch"].kind == inspect.Parameter.KEYWORD_ONLY and params["batch"].default is False
    assert params["seed"].kind == inspect.Parameter.KEYWORD_ONLY and params["seed"].default is None


def _estimate(moments_fn=None):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    from mlmc_amd.sample_storage import Memory
    spec = [QuantitySpec(name="q", unit="m", shape=(1, 1), times=[1], locations=['0'])]
    st = Memory()
    st.save_global_data(result_format=spec, level_parameters=[[0.5], [0.1]])
    rng = np.random.default_rng(5)
    st.set_level_samples(0, rng.normal(size=(50, 1)), None)
    st.set_level_samples(1, rng.normal(size=(20, 1)), rng.normal(size=(20, 1)))
    q = make_root_quantity(st, spec)['q'][1]['0'][0, 0]
    return Estimate(q, st, moments_fn if moments_fn is not None else Legendre(4, (-3.0, 3.0)))


def _no_device(monkeypatch):
    from mlmc_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(_lib, "lib", no_device)
    monkeypatch.setattr(_lib, "init", no_device)


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
])
def test_bootstrap_batch_argument_errors_before_the_device(monkeypatch, kwargs, match):
    est = _estimate()
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match=match):
        est.est_bootstrap_batch(**kwargs)


def test_bootstrap_batch_rejects_splines_and_transformed_moments(monkeypatch):
    from mlmc_amd import Legendre
    from mlmc_amd.moments import Spline, TransformedMoments
    est = _estimate()
    _no_device(monkeypatch)
    for fn in (Spline(6, (-3.0, 3.0)), TransformedMoments(Legendre(4, (-3.0, 3.0)), np.eye(3, 4))):
        with pytest.raises(ValueError, match="est_bootstrap"):
            est.est_bootstrap_batch(10, moments_fn=fn)


def test_bootstrap_sizes_prefix_and_keys():
    from mlmc_amd.quantity import quantity_estimate as qe
    a = qe.bootstrap_sizes(77, 2, 1, 400, 1000, 300, 300)
    b = qe.bootstrap_sizes(77, 2, 1, 400, 1000, 300, 50)
    assert a.dtype == np.int64 and a.shape == (300,) and np.array_equal(a[:50], b)
    assert np.array_equal(a, qe.bootstrap_sizes(77, 2, 1, 400, 1000, 300, 300))
    # keyed by (seed, level, chunk): another key gives other draws
    for other in ((78, 2, 1), (77, 3, 1), (77, 2, 2)):
        assert not np.array_equal(a, qe.bootstrap_sizes(*other, 400, 1000, 300, 300))
    # the parameters of the loop: good = k, bad = N - k, draws = min(n_c, N)
    assert np.all((a >= 0) & (a <= 300))
    assert abs(np.mean(a) - 300 * 400 / 1000) < 4 * np.sqrt(300 * 0.4 * 0.6 * 700 / 999 / 300) + 1.0
    assert np.all(qe.bootstrap_sizes(1, 0, 0, 0, 500, 200, 20) == 0)
    assert np.all(qe.bootstrap_sizes(1, 0, 0, 500, 500, 200, 20) == 200)
    assert qe.bootstrap_stream(3, 5) == (3 << 20) | 5
