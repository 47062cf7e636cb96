"""CPU tests of the component covariance (quantity_estimate.component_covariance): the node's qtype, the argument errors that
come before any device call, and the new C-ABI symbols in header, binding and library."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _root_quantity(M_arr=3, times=(1, 2)):
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    from mlmc_amd.sample_storage import Memory
    spec = [QuantitySpec(name="q", unit="m", shape=(M_arr, 1), times=list(times), locations=['0'])]
    st = Memory()
    st.save_global_data(result_format=spec, level_parameters=[[0.1], [0.01]])
    rng = np.random.default_rng(3)
    M = M_arr * len(times)
    st.set_level_samples(0, rng.normal(size=(20, M)))
    st.set_level_samples(1, rng.normal(size=(10, M)), rng.normal(size=(10, M)))
    return make_root_quantity(st, spec)['q'], M


def test_node_qtype_and_shape():
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.quantity import quantity_types as qt
    q, M = _root_quantity()
    node = qe.component_covariance(q)
    assert isinstance(node.qtype, qt.ArrayType) and node.qtype._shape == (M, M)
    assert isinstance(node.qtype._qtype, qt.ScalarType)
    assert node.size() == M * M
    assert node._shift is None
    node = qe.component_covariance(q, shift=np.arange(M))
    assert node._shift.dtype == np.float64 and np.array_equal(node._shift, np.arange(M))
    # a scalar component is a quantity of one component
    one = qe.component_covariance(q[1]['0'][0, 0])
    assert one.qtype._shape == (1, 1)
    with pytest.raises(NotImplementedError):
        node._eval(np.zeros((M, 3, 2)))


def test_argument_errors_before_any_device_call(monkeypatch):
    from mlmc_amd import _lib
    from mlmc_amd.quantity import quantity_estimate as qe

    def no_device(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(_lib, "lib", no_device)
    monkeypatch.setattr(_lib, "init", no_device)
    q, M = _root_quantity()
    with pytest.raises(ValueError, match="shift"):
        qe.component_covariance(q, shift=np.zeros(M + 1))
    with pytest.raises(ValueError, match="shift"):
        qe.component_covariance(q, shift=np.zeros((M, 1)))
    with pytest.raises(ValueError, match="finite"):
        qe.component_covariance(q, shift=np.full(M, np.nan))
    big, M_big = _root_quantity(M_arr=513, times=(1, 2))
    assert M_big == 1026
    with pytest.raises(ValueError, match="1024"):
        qe.component_covariance(big)
    for bad in (np.zeros((3, 4)), [1.0, 2.0], None):
        with pytest.raises(TypeError):
            qe.component_covariance(bad)
    from mlmc_amd import Legendre
    with pytest.raises(TypeError):
        qe.component_covariance(qe.moments(q, Legendre(3, (-1.0, 1.0))))
    with pytest.raises(TypeError):
        qe.component_covariance(qe.component_covariance(q))
    from mlmc_amd.engine import ComponentCovAccumulator
    with pytest.raises(ValueError, match="1024"):
        ComponentCovAccumulator(1025, 2)
    with pytest.raises(ValueError, match="1024"):
        ComponentCovAccumulator(0, 2)


def test_new_symbols_in_header_binding_and_library():
    from mlmc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mlmc_hip.h")).read()
    assert int(re.search(r"#define MLMC_ABI_VERSION (\d+)", hdr).group(1)) == 8 == _lib.ABI_VERSION
    lib = _lib.load()
    assert lib.mlmc_abi_version() == 8
    for name in ("mlmc_xcov_create", "mlmc_xcov_set_shift"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)


def test_estimate_method_exists():
    from mlmc_amd.estimator import Estimate
    assert callable(getattr(Estimate, "estimate_component_covariance", None))
