"""Case table of tests/test_gpu_latw_bits.py and of scripts/record_latw_bits.py: the smallest shape per schedule of the latency round
(pympc_amd/csrc/mpcqp_latw.h), what is computed for each and where its recorded bits live."""
import os

import numpy as np

from util import GOLDEN_DIR, stacked_batch, forced

BITS_DIR = os.path.join(GOLDEN_DIR, 'latw_bits')
BATCH = 2
ITERS = (1, 7, 25)          # one mpcqp_iterate call each, on one handle: the iterate is read after 1, 8 and 33 iterations

# name -> (nx, nu, Np, backend, mode in the kernel's name)
CASES = {
    'spec_12_4_30_bcr8': (12, 4, 30, 'bcr8', 231),       # the specialised instantiation of the headline shape: 31 stages on eight waves, fused schedule
    'gen_5_3_28_bcr8': (5, 3, 28, 'bcr8', 231),          # the generic instantiation of the same schedule, 29 of its 31 stages in use
    'gen_4_2_20_bcr8': (4, 2, 20, 'bcr8', 221),          # 21 stages: seven barriers, waves share groups of stages
    'gen_4_2_10_bcr8': (4, 2, 10, 'bcr8', 211),          # 11 stages
    'spec_12_4_30_bcrt': (12, 4, 30, 'bcrt', 231),       # the 256-thread build: four waves, two groups of stages per wave
}


def compute(name):
    """{'x1', 'z1', 'y1', 'x7', ...}: the iterate of a batch of BATCH random plants after each of the ITERS calls, and the kernel's name."""
    from pympc_amd import fixtures
    nx, nu, Np, backend, mode = CASES[name]
    kws = [fixtures.random_lti(4100 + 17 * nx + i, nx=nx, nu=nu, Np=Np, xbox=10.0) for i in range(BATCH)]
    out = {}
    with forced(backend=backend):
        K = stacked_batch(kws, Nc=None, eps_feas=1e6)
        K.setup(solve=False)
        kn = K.prob.kernel_name(loop=False)
        for k in ITERS:
            K.prob.iterate(k)
            for tag, v in zip('xzy', K.prob.iterate_state()):
                out['%s%d' % (tag, k)] = np.array(v)
    return out, kn


def path(name):
    return os.path.join(BITS_DIR, name + '.npz')
