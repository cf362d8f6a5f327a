"""The recorded runs of tests/test_gpu_latw_boundary_bits.py take every exit of the round boundary (tests/latw_boundary_cases.py: assert_classes) and
were fed what the table says: conditions on the goldens and on the case table, checked without a GPU."""
import os

import numpy as np

from latw_boundary_cases import CASES, FLOAT_KEYS, INT_KEYS, assert_classes, inputs, kernel_suffix, path


def test_recorded_runs_take_every_exit():
    cs = assert_classes({name: np.load(path(name)) for name in CASES})
    assert sorted(cs) == sorted(CASES)


def test_goldens_are_small_and_complete():
    for name in CASES:
        assert os.path.getsize(path(name)) < 100 * 1024, name
        g = np.load(path(name))
        assert sorted(g.files) == sorted(FLOAT_KEYS + INT_KEYS + ('kernel',)), (name, g.files)
        assert str(g['kernel']).endswith(kernel_suffix(name)), (name, str(g['kernel']))


def test_weights_are_dense_and_terminal_weight_differs():
    plants = 0
    for name, (nx, nu, Np, hard, own_plant) in CASES.items():
        kws, w, (Ap, Bp) = inputs(name)
        assert (Ap is not None) == own_plant and (Bp is not None) == own_plant, name
        plants += own_plant
        for kw in kws:
            for k in ('Qx', 'QxN', 'Qu', 'QDu'):
                Q = np.asarray(kw[k])
                assert np.array_equal(Q, Q.T) and (Q != 0.0).all() and np.linalg.eigvalsh(Q).min() > 0.0, (name, k)
            assert not np.array_equal(kw['Qx'], kw['QxN']), name
            assert 'Nc' not in kw, name
    assert plants >= 1
