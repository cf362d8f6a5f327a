"""The latency round's check and carry get the instance they work on BY VALUE from admm_latw (pympc_amd/csrc/mpcqp_latw_check.h) instead of
loading the workgroup -> instance map again.  What that can break: a workgroup of a PERSISTENT launch that goes on working on the instance of its
previous queue item after the queue has handed it a new one.  So: three instances more than there are resident slots (every workgroup takes
several items, some of them of different instances), every instance's loop cut into at least two items, distinct plants under process noise --
against the same loop with one workgroup per instance (MPCQP_TUNE_NO_QUEUE: no queue, no map to get wrong) and against the loop that leaves the
round after every solve (MPCQP_TUNE_NO_CARRY), bit for bit.  One instance receives a NaN disturbance: its carry hands the step back to the
kernel's begin (tests/test_gpu_loop_carry.py), and its neighbours in the queue must not notice.
Run on the GPU box with:  python -m pytest tests -m gpu
"""
import warnings

import numpy as np
import pytest

from util import stacked_batch, forced

pytestmark = pytest.mark.gpu

NX, NU, NP = 4, 2, 21           # 22 stages: the generic instantiation of the 31-stage schedule, eight waves
STEPS = 6
NOISE = 0.02
BAD, BAD_STEP = 5, 2            # the instance whose disturbance of step 2 is not a number
ITEMS = 2                       # development override: queue items per resident slot -> ceil(2 * slots / (slots + 3)) = 2 parts per instance


def _slots():
    """Resident workgroup slots of the forced kernel on this device, from a one-instance handle's mpcqp_get_occupancy."""
    from pympc_amd import fixtures
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with forced(backend='bcr8'):
            K = stacked_batch([fixtures.random_lti(7700, nx=NX, nu=NU, Np=NP)], Nc=None, eps_feas=1e6)
            K.setup(solve=False)
    occ, ncu, threads = K.prob.occupancy()
    assert threads == 512 and occ >= 1 and ncu >= 1, (occ, ncu, threads)
    return occ * ncu


def _run(kws, w, tuning):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with forced(backend='bcr8', tuning=tuning):
            K = stacked_batch(kws, Nc=None, eps_feas=1e6, max_iter=2000)
            K.setup()
        kn = K.prob.kernel_name(True).replace(' ', '')
        assert kn.startswith('w8::k_mpc_run<16,') and kn.endswith(',0,0,231,true>'), kn
        r = K.run(STEPS, w=w)
    return {k: np.array(r[k]) for k in ('x', 'u', 'status', 'iter')}, K.prob.carry_stats()


def test_queue_items_keep_their_instance():
    from pympc_amd import fixtures, _lib
    B = _slots() + 3
    kws = [fixtures.random_lti(7700 + i, nx=NX, nu=NU, Np=NP) for i in range(B)]
    w = np.stack([NOISE * fixtures.random_lti_noise_rng(7700 + i).standard_normal((STEPS, NX)) for i in range(B)], axis=1)
    w[BAD_STEP, BAD, 0] = np.nan
    items = ITEMS << _lib.TUNE_ITEMS_SHIFT
    a, (carried, back, parts) = _run(kws, w, items)
    # the launch this test is about: persistent, every instance in at least two items, steps carried inside the round, one handed back
    assert parts >= 2, parts
    assert carried > B and back >= 1, (carried, back)
    others = [i for i in range(B) if i != BAD]
    assert np.isnan(a['x'][BAD_STEP + 1:, BAD]).any() and np.isfinite(a['x'][:, others]).all() and np.isfinite(a['u'][:, others]).all()
    assert (a['status'][:, others] == 1).mean() > 0.9 and a['iter'][:, others].min() > 0
    plants = a['x'][1:, others].reshape(STEPS, len(others), NX)
    assert len({plants[:, i].tobytes() for i in range(len(others))}) == len(others)      # (distinct plants: a wrong instance cannot pass for the right one)
    for name, tuning in (('no queue', _lib.TUNE_NO_QUEUE), ('no carry', items | _lib.TUNE_NO_CARRY)):
        b, (carried_b, back_b, parts_b) = _run(kws, w, tuning)
        if tuning & _lib.TUNE_NO_CARRY:
            assert (carried_b, back_b) == (0, 0) and parts_b == parts, (carried_b, back_b, parts_b)
        else:
            assert parts_b == 0 and carried_b > B, (carried_b, parts_b)                  # (one workgroup per instance: the whole loop may be carried)
        for k in ('x', 'u', 'status', 'iter'):
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (name, k)
            assert np.array_equal(a[k][:, others], b[k][:, others]), (name, k)           # the neighbours: every bit
            assert np.array_equal(a[k], b[k], equal_nan=True), (name, k)                 # ... and the instance that went non-finite
