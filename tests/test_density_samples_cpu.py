"""CPU tests of the sampling entry: the NumPy restatement of its uniforms (tests/sample_cases.py) against the Random123
known-answer vectors and its own definition, a DKW bound on the uniforms, and the boundary of the new entry (declared, bound,
exported, ABI version unchanged; no CPU fallback of the Python entries)."""
import os
import re

import numpy as np
import pytest

from tests import sample_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "mlmc_density_sample_batch"
PAIRS = [(7, s) for s in (0, 1, 2, 11)]


def test_known_answers():
    """the three Philox4x32-10 vectors of Random123's kat_vectors"""
    ones = 0xFFFFFFFF
    for counter, key, want in (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                               ((ones,) * 4, (ones, ones), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                               ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                                (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        got = sc.philox4x32_10(counter, key)
        assert tuple(int(v) for v in got) == want, [hex(int(v)) for v in got]
    # arrays give what scalars give
    got = sc.philox4x32_10((np.array([0, ones, 0x243f6a88]), np.array([0, ones, 0x85a308d3]), np.array([0, ones, 0x13198a2e]),
                            np.array([0, ones, 0x03707344])), (0, 0))
    assert int(got[0][0]) == 0x6627e8d5 and got[0].shape == (3,)


def test_first_uniforms():
    """recorded first values (seed 7: stream 0 begins 0.07114859, stream 3 begins 0.57088122), and the definition by hand"""
    u = sc.uniforms(7, 0, 0, 3)
    assert np.allclose(u, [0.07114859, 0.98634542, 0.25290859], rtol=0, atol=5e-9), u
    assert np.allclose(sc.uniforms(7, 3, 0, 3), [0.57088122, 0.81913212, 0.45926162], rtol=0, atol=5e-9)
    # the definition by hand for uniform 0 and 1 of the stream: one Philox call, words (r0, r1) and (r2, r3)
    r = [int(v) for v in sc.philox4x32_10((0, 0, 0, sc.TAG), (7, 0))]
    for k, (hi, lo) in enumerate(((r[0], r[1]), (r[2], r[3]))):
        m = (hi << 20) | (lo >> 12)
        assert u[k] == (2 * m + 1) / 2.0 ** 53 and m < 2 ** 52


def test_uniforms_are_odd_multiples():
    """odd multiples of 2^-53 inside (0, 1), and 1 - u is exact: (1 - u) + u == 1"""
    for seed, stream, first in ((7, 0, 0), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 33 + 1), (0, 5, 2 ** 62)):
        for anti in (False, True):
            u = sc.uniforms(seed, stream, first, 4096, anti)
            k = u * 2.0 ** 53
            assert np.all(k == np.floor(k)) and np.all(k.astype(np.int64) % 2 == 1)
            assert np.all(u > 0) and np.all(u < 1)
            assert np.all((1.0 - u) + u == 1.0)
            assert len(np.unique(u)) == u.size


def test_slices_agree_with_the_whole():
    for anti in (False, True):
        whole = sc.uniforms(7, 3, 0, 150, anti)
        assert np.array_equal(sc.uniforms(7, 3, 50, 100, anti), whole[50:150])
        assert np.array_equal(sc.uniforms(7, 3, 149, 1, anti), whole[149:])
        assert sc.uniforms(7, 3, 10, 0, anti).size == 0
        far = 2 ** 33 + 1                               # the high counter word, an odd start
        whole = sc.uniforms(7, 3, far - 1, 12, anti)
        assert np.array_equal(sc.uniforms(7, 3, far, 11, anti), whole[1:])
    # the high word of the index reaches the counter; streams and seeds differ
    assert not np.array_equal(sc.uniforms(7, 3, 2 ** 33, 8), sc.uniforms(7, 3, 0, 8))
    assert not np.array_equal(sc.uniforms(7, 3, 0, 8), sc.uniforms(7, 4, 0, 8))
    assert not np.array_equal(sc.uniforms(7, 3, 0, 8), sc.uniforms(7 + 2 ** 32, 3, 0, 8))
    assert not np.array_equal(sc.uniforms(7, 3, 0, 8), sc.uniforms(8, 3, 0, 8))


def test_antithetic_pairs():
    for first in (0, 1, 2 ** 33 + 1):
        u = sc.uniforms(7, 2, first, 1001, True)
        j = first + np.arange(1001)
        even = np.where(j % 2 == 0)[0]
        even = even[even + 1 < u.size]
        assert np.array_equal(u[even + 1], 1.0 - u[even])
    # draw 2k of the antithetic sequence is uniform k of the plain one
    assert np.array_equal(sc.uniforms(7, 2, 0, 1000, True)[::2], sc.uniforms(7, 2, 0, 500))


def test_dkw_bound_on_the_uniforms():
    """Kolmogorov distance of 16384 uniforms from U(0, 1) at most sqrt(ln(2 / 1e-9) / (2 n)) = 0.02557, the DKW bound at
    confidence 1 - 1e-9: a condition, not a measurement (the reference alone gives 0.0044 .. 0.0119)"""
    assert abs(sc.DKW_BOUND - 0.02557) < 5e-6
    print()
    for seed, stream in PAIRS:
        d = sc.kolmogorov_distance(sc.uniforms(seed, stream, 0, sc.DKW_N))
        print(f"seed {seed} stream {stream:2d}: Kolmogorov distance {d:.4f} (bound {sc.DKW_BOUND:.5f})")
        assert d <= sc.DKW_BOUND, (seed, stream, d)
    assert sc.kolmogorov_distance(np.linspace(0, 0.5, 1000)) > 0.49          # the distance sees a wrong distribution


def test_entry_is_declared_bound_and_exported():
    from mlmc_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "mlmc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+" + ENTRY + r"\s*\(", code)
    assert re.search(r"#define\s+MLMC_SAMPLE_ANTITHETIC\s+1\b", code) and _lib.SAMPLE_ANTITHETIC == 1
    assert ENTRY in _lib.SIGNATURES and hasattr(lib, ENTRY)
    comment = text.split("#define MLMC_ABI_VERSION")[1].split("*/")[0]
    assert ENTRY in comment.split("added within 8")[1], ENTRY + " is not named in the version comment"
    assert len(_lib.SIGNATURES[ENTRY][1]) == 18
    assert _lib.ABI_VERSION == 8 and lib.mlmc_abi_version() == 8
    assert re.search(r"#define\s+MLMC_ABI_VERSION\s+8\b", text)
    timing = text.split("int mlmc_density_quantiles_kernel_time")[0].rsplit("/*", 1)[1]
    assert ENTRY in timing, "the comment of mlmc_density_quantiles_kernel_time does not name the sampling kernel"


def _distributions():
    from mlmc_amd import Legendre
    from mlmc_amd.tool import simple_distribution as sd
    from mlmc_amd.tool.distribution import Distribution
    dom = (-1.0, 1.0)
    data = np.stack([np.eye(4)[0], np.ones(4)], axis=1)
    d = sd.SimpleDistribution(Legendre(4, dom), data, domain=dom)
    d._initialize_params(4, 1e-8)
    old = Distribution(Legendre(4, dom), data.copy(), domain=dom)
    old.multipliers, old._moment_errs = d.multipliers, d.moment_errs
    return d, old


def test_no_cpu_fallback_of_the_new_entries():
    """argument checks of the Python layer, and without a device the new entries raise like every other compute call"""
    import torch
    from mlmc_amd import _lib
    from mlmc_amd.tool import simple_distribution as sd
    assert sd.samples([], 5, seed=1) == [] and sd.samples([], 5, seed=1, return_uniforms=True) == ([], [])
    d, old = _distributions()
    with pytest.raises(TypeError):
        d.rvs(5)                                        # seed is required
    for bad_seed in (None, -1, 2 ** 64, 0.5, True):
        with pytest.raises(ValueError, match="seed"):
            sd.samples([d], 5, seed=bad_seed)
    with pytest.raises(ValueError, match="n must be"):
        sd.samples([d, d], [1, 2, 3], seed=1)
    with pytest.raises(ValueError, match="n must be"):
        sd.samples([d], -1, seed=1)
    with pytest.raises(ValueError, match="first must be"):
        sd.samples([d], 1, seed=1, first=-1)
    with pytest.raises(ValueError, match="streams"):
        sd.samples([d, d], 1, seed=1, streams=[0])
    with pytest.raises(ValueError, match="streams"):
        sd.samples([d], 1, seed=1, streams=[2 ** 32])
    other = _distributions()[0]
    other.n_intervals = 200
    with pytest.raises(ValueError, match="same quadrature"):
        sd.samples([d, other], 1, seed=1)
    if torch.cuda.is_available():
        return
    for call in (lambda: sd.samples([d], 5, seed=1), lambda: sd.samples([d, d], [1, 2], seed=1, device=True),
                 lambda: d.rvs(5, 1), lambda: d.rvs(5, seed=1, stream=3, first=2, antithetic=True), lambda: old.rvs(5, seed=1)):
        with pytest.raises(_lib.MlmcHipError):
            call()


def test_estimate_entry_without_a_device():
    import torch
    from mlmc_amd import _lib, estimator
    assert callable(estimator.Estimate.sample_components)
    assert "independent" in estimator.Estimate.sample_components.__doc__.lower()
    assert "quantiles" in estimator.Estimate.sample_components.__doc__
    est = estimator.Estimate(None, None, None)
    d = _distributions()[0]
    densities = [(d, None, type("R", (), {"success": True})(), None)]
    with pytest.raises(TypeError):
        est.sample_components(5, densities=densities)   # seed is required
    with pytest.raises(ValueError, match="n must be"):
        est.sample_components(-5, 1, densities=densities)
    if torch.cuda.is_available():
        return
    with pytest.raises(_lib.MlmcHipError):
        est.sample_components(5, 1, densities=densities)
