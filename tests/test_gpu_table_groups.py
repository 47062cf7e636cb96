"""GPU test of the groups of the table bound in the entries that make their draws or scores per group of problems:
mlmc_density_sample_joint_batch, mlmc_density_sample_conditional_batch (one host path, q_copula in mlmc_amd/csrc/density.hip) and
mlmc_density_scores_batch (q_scores).

A call whose P rows exceed the table bound of 64 MiB runs in groups of problems that share the table in stream order.  The joint
and the conditional entry then regenerate the latent normals of a block per group (workspace) or read them back from the caller's
device array, and copy the uniforms of a group back per block.  Every row must be bit for bit the row of a call that holds the
problems of its group alone."""
import os

import numpy as np
import pytest

from tests import joint_sample_cases as jc
from tests.test_gpu_conditional_samples import SENTINEL, _cok, _scaled_factor
from tests.test_gpu_density_samples import _same
from tests.test_gpu_joint_samples import _cycle, _ok, hip, table  # noqa: F401  (fixtures)
from tests.test_gpu_normal_scores import _ok as _sok, _points

pytestmark = pytest.mark.gpu
QUAD = (1 << 20, 5)                    # one P row is 8 MiB and 8 bytes; the low degree keeps the tables cheap
M, N, BLOCK = 8, 130, 64               # two groups of 7 and 1 problems; three blocks of 64, 64 and 2 draws
PARTS = (slice(0, 7), slice(7, 8))


@pytest.fixture(scope="module")
def group(table):
    """eight problems of the sampling tests' cases on the rule QUAD"""
    row = 8 * (QUAD[0] + 1)
    assert row * M > (64 << 20) >= row * 7 and (64 << 20) // row == 7
    return [dict(p, quad=QUAD) for p in _cycle(table[0], M)]


@pytest.fixture()
def blocks():
    """MLMC_JOINT_BLOCK_DRAWS = BLOCK for the test"""
    assert "MLMC_JOINT_BLOCK_DRAWS" not in os.environ and N > 2 * BLOCK and N % BLOCK
    os.environ["MLMC_JOINT_BLOCK_DRAWS"] = str(BLOCK)
    try:
        yield
    finally:
        del os.environ["MLMC_JOINT_BLOCK_DRAWS"]


@pytest.mark.parametrize("kind", ["host", "device"])
def test_joint_groups(hip, group, blocks, kind):
    """rows 0..6 are the call on the first seven problems, row 7 the call on the eighth; z_out is that of either.  With device
    arrays u_out and z_out are written in place, and the second group reads the normals the first has left in z_out"""
    kind = hip.HOST if kind == "host" else hip.DEVICE
    F = jc.random_factor(np.random.default_rng(31), M, 3)
    out, u, z, mass = _ok(hip, group, F, N, first=5, kind=kind, want_mass=True)
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(z)) and np.all((u > 0) & (u < 1)) and np.all(mass > 0)
    for part in PARTS:
        o, uu, zz, mm = _ok(hip, group[part], F[part], N, first=5, kind=kind, want_mass=True)
        assert _same(o, out[part]) and _same(uu, u[part]) and _same(zz, z) and np.array_equal(mm, mass[part]), part


@pytest.mark.parametrize("kind", ["host", "device"])
def test_conditional_groups(hip, group, blocks, kind):
    """the same with two sets, a shift, rows with gaps and ld_rows = M + 2; the rows that `rows` does not name keep their sentinel"""
    kind = hip.HOST if kind == "host" else hip.DEVICE
    rng = np.random.default_rng(32)
    F = _scaled_factor(rng, M, 3)
    shift = rng.uniform(-2.0, 2.0, (2, M))
    rows = np.array([0, 1, 3, 4, 5, 6, 8, 9])
    gaps = np.setdiff1d(np.arange(M + 2), rows)
    out, u, z, mass = _cok(hip, group, F, N, B=2, shift=shift, rows=rows, ld_rows=M + 2, first=5, kind=kind, want_mass=True)
    assert out.shape == (2, M + 2, N) and np.all(np.isfinite(out[:, rows])) and np.all((u[:, rows] > 0) & (u[:, rows] < 1))
    assert np.all(out[:, gaps] == SENTINEL) and np.all(u[:, gaps] == SENTINEL) and not _same(out[0, rows], out[1, rows])
    for part in PARTS:
        o, uu, zz, mm = _cok(hip, group[part], F[part], N, B=2, shift=shift[:, part], rows=rows[part], ld_rows=M + 2, first=5,
                             kind=kind, want_mass=True)
        named = rows[part]
        assert _same(o[:, named], out[:, named]) and _same(uu[:, named], u[:, named]) and _same(zz, z), part
        assert np.array_equal(mm, mass[part]), part
        other = np.setdiff1d(np.arange(M + 2), named)
        assert np.all(o[:, other] == SENTINEL) and np.all(uu[:, other] == SENTINEL), part


def test_scores_groups(hip, group):
    """[8][n] stored samples with a coarse array: rows 0..6 and row 7 are the calls on those problems"""
    rng = np.random.default_rng(33)
    fine, coarse = _points(rng, group, N), _points(rng, group, N)
    whole = _sok(hip, group, fine, coarse, quad=QUAD, want_mass=True)
    assert np.isfinite(whole[0]).sum() > M * (N - 4) and np.all(whole[4] > 0)
    for part in PARTS:
        got = _sok(hip, group[part], fine[part], coarse[part], quad=QUAD, want_mass=True)
        assert all(_same(g, w[part]) for g, w in zip(got[:4], whole[:4])) and np.array_equal(got[4], whole[4][part]), part
