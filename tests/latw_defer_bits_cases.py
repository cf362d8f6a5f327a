"""Case table of tests/test_gpu_latw_defer_bits.py and of scripts/record_latw_defer_bits.py: what the fused schedule of the latency round
(pympc_amd/csrc/mpcqp_latw.h) can break when a leaf product D^-1 b runs a phase later -- tb at 4r+1 (4w, 4w+2 for level 0's leaves) is then read,
and cb written, a phase later than the value was made -- on the shapes tests/latw_bits_cases.py does not have: the 31-stage template with most trailing stages
absent, a shape whose owner lanes are mostly dead, and closed loops that carry steps and cross round boundaries inside the kernel, where the
termination test and the carry reuse the round's LDS vectors."""
import os

import numpy as np

from util import GOLDEN_DIR, stacked_batch, forced

BITS_DIR = os.path.join(GOLDEN_DIR, 'latw_defer_bits')
BATCH = 2
ITERS = (1, 7, 25)          # one mpcqp_iterate call each, on one handle: the iterate is read after 1, 8 and 33 iterations
STEPS = 6                   # closed-loop steps of a 'loop_' case, in one mpc_run
NOISE = 0.02                # standard deviation of its process noise

# name -> (nx, nu, Np, backend, mode in the kernel's name); 'iter_': plain iterations, 'loop_': the device loop
CASES = {
    'iter_4_2_21_bcr8': (4, 2, 21, 'bcr8', 231),         # 22 stages: the fewest the 31-stage schedule serves, waves 6 and 7 own absent stages only
    'iter_3_1_30_bcr8': (3, 1, 30, 'bcr8', 231),         # every stage present, four of sixteen owner lanes alive
    'loop_12_4_30_bcr8': (12, 4, 30, 'bcr8', 231),       # the specialised instantiation through step carries and round boundaries
    'loop_4_2_21_bcr8': (4, 2, 21, 'bcr8', 231),         # ... and the generic one with trailing stages absent
}


def _controllers(name):
    from pympc_amd import fixtures
    nx, nu, Np, backend, mode = CASES[name]
    return [fixtures.random_lti(5200 + 17 * nx + i, nx=nx, nu=nu, Np=Np, xbox=10.0) for i in range(BATCH)]


def compute(name):
    """The arrays of one case and the kernel's name.  'iter_': {'x1', 'z1', 'y1', 'x7', ...}, the iterate of BATCH random plants after each of the
    ITERS calls;  'loop_': x, u, status and iter of STEPS closed-loop steps under process noise."""
    from pympc_amd import fixtures
    nx, nu, Np, backend, mode = CASES[name]
    kws = _controllers(name)
    out = {}
    with forced(backend=backend):
        if name.startswith('iter_'):
            K = stacked_batch(kws, Nc=None, eps_feas=1e6)
            K.setup(solve=False)
            kn = K.prob.kernel_name(loop=False)
            for k in ITERS:
                K.prob.iterate(k)
                for tag, v in zip('xzy', K.prob.iterate_state()):
                    out['%s%d' % (tag, k)] = np.array(v)
        else:
            K = stacked_batch(kws, Nc=None, eps_feas=1e6)
            K.setup()
            kn = K.prob.kernel_name(loop=True)
            w = np.stack([NOISE * fixtures.random_lti_noise_rng(5200 + i).standard_normal((STEPS, nx)) for i in range(BATCH)], axis=1)
            r = K.run(STEPS, w=w)
            for k in ('x', 'u', 'status', 'iter'):
                out[k] = np.array(r[k])
            out['carried'] = np.array(K.prob.carry_stats()[0])
    return out, kn


def path(name):
    return os.path.join(BITS_DIR, name + '.npz')
