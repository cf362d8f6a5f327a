"""The Python layer above the four taped loops (pympc_amd/solver.py, pympc_amd/torch_layer.py, pympc_amd/batch.py) calls the library with the
arguments and adds torch's tensors up in the order it did when tests/golden/rollout_layer_bits.npz was recorded
(scripts/record_rollout_layer_bits.py says what is in it): every output and every gradient of mpc_rollout, mpc_rollout_est, mpc_rollout_tv and
mpc_rollout_tv_est, and every name rollout_adjoint takes on each of the four tapes, bit for bit."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_four_forms_have_the_bits_they_had():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import record_rollout_layer_bits as rec
    finally:
        sys.path.pop(0)
    gold = rec.load(os.path.join(ROOT, 'tests', 'golden', 'rollout_layer_bits.npz'))
    got = rec.outputs()
    assert sorted(gold) == sorted(got)
    for form in rec.FORMS:                                 # (every form is there with both of its faces and a gradient that is not zero)
        assert np.abs(gold[form + '.batch.Ad']).max() > 0.0 and np.abs(gold[form + '.b.d_params_Bd']).max() > 0.0
    for k in gold:
        assert got[k].dtype == gold[k].dtype and got[k].shape == gold[k].shape and np.array_equal(got[k], gold[k]), k
