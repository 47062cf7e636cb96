"""CPU tests of the host side of Estimate.construct_densities: the scalar sub-quantity of row m of a vector quantity
(estimator.scalar_component) and its row order."""
import numpy as np


def _storage():
    from mlmc_amd.sample_storage import Memory
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    rng = np.random.default_rng(5)
    spec = [QuantitySpec(name="a", unit="m", shape=(3, 2), times=[1, 2], locations=['0', '1']),
            QuantitySpec(name="b", unit="m", shape=(1, 1), times=[1], locations=['0'])]
    st = Memory()
    st.save_global_data(result_format=spec, level_parameters=[[0.1], [0.01]])
    n_rows = 2 * 2 * 6 + 1
    st.set_level_samples(0, rng.normal(size=(50, n_rows)))
    st.set_level_samples(1, rng.normal(size=(30, n_rows)), rng.normal(size=(30, n_rows)))
    return st, spec


def test_scalar_component_rows_and_order():
    from mlmc_amd.estimator import scalar_component
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.quantity.quantity_types import ScalarType
    st, spec = _storage()
    root = make_root_quantity(st, spec)
    assert root.size() == 25
    a = root['a']
    for level_id in (0, 1):
        chunk = next(st.chunks(level_id=level_id))
        whole = root.samples(chunk)
        for m in range(25):
            q_m = scalar_component(root, m)
            assert isinstance(q_m.qtype, ScalarType) and q_m.size() == 1
            assert np.array_equal(q_m.samples(chunk), whole[m:m + 1])
        # dict 'a' -> time -> location -> array (3, 2) row-major: m = (t * 2 + loc) * 6 + i * 2 + j
        for ti, t in enumerate((1, 2)):
            for li, loc in enumerate(('0', '1')):
                for i in range(3):
                    for j in range(2):
                        m = (ti * 2 + li) * 6 + i * 2 + j
                        assert np.array_equal(a[t][loc][i, j].samples(chunk), whole[m:m + 1])
        arr = a[2]['1']                                    # an ArrayType quantity: its own rows, unravelled
        for k in range(6):
            assert np.array_equal(scalar_component(arr, k).samples(chunk), arr.samples(chunk)[k:k + 1])
        assert np.array_equal(root['b'][1]['0'][0, 0].samples(chunk), whole[24:25])
