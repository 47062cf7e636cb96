"""CPU tests of the per-component domains: the new C-ABI entry in header, binding and library, the Python entry points, and the
shape errors of engine.row_percentiles that come before any device call."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_percentiles_symbol_in_header_binding_and_library():
    from mlmc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mlmc_hip.h")).read()
    assert re.search(r"\bmlmc_percentiles_rows\s*\(", hdr)
    assert "mlmc_percentiles_rows" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["mlmc_percentiles_rows"]
    assert len(args) == 9
    assert hasattr(_lib.load(), "mlmc_percentiles_rows")


def test_abi_version_stays_8():
    from mlmc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mlmc_hip.h")).read()
    assert int(re.search(r"#define MLMC_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert _lib.ABI_VERSION == 8 and _lib.load().mlmc_abi_version() == 8


def test_estimate_domains_entry_points_exist():
    from mlmc_amd import estimator
    from mlmc_amd.estimator import Estimate
    assert callable(getattr(Estimate, "estimate_domains", None))
    assert callable(getattr(estimator, "estimate_domains", None))
    from mlmc_amd import engine
    assert callable(getattr(engine, "row_percentiles", None))


@pytest.mark.parametrize("shape", [(5,), (2, 3, 4), ()])
def test_row_percentiles_rejects_other_ranks_before_the_library(monkeypatch, shape):
    from mlmc_amd import _lib, engine

    def no_device(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(_lib, "lib", no_device)
    monkeypatch.setattr(_lib, "init", no_device)
    with pytest.raises(ValueError, match="2-D"):
        engine.row_percentiles(np.zeros(shape), [1.0, 99.0])
    import torch
    with pytest.raises(ValueError, match="2-D"):
        engine.row_percentiles(torch.zeros(shape, dtype=torch.float64), [1.0, 99.0])
