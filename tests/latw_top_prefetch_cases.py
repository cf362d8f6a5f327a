"""Case table of tests/test_gpu_latw_top_prefetch_bits.py and of scripts/record_latw_top_prefetch_bits.py: the top of the latency round
(pympc_amd/csrc/mpcqp_latw.h, latw_top_valu) under a regrouping of its LDS requests.  The top fetches the column pairs of a wave's block row of the
top inverse in fenced groups -- single pairs with eight waves, where the goldens' library fetched two at a time -- and any other grouping or earlier
request of them (one was measured and not kept: LAB_NOTES.md) has to pass here too.  No summand and no order of a sum moves; what a regrouping can
break is a pair taken from the wrong row or column, a column pair summed twice or not at all where two groups meet, a value that outlives a rewrite
of the inverse, and a wave without a top row.  Closed loops of BATCH instances x STEPS steps in one mpc_run, per case:

    first_12_4_30      the fused schedule (eight waves, one group of four stages each; NTOP = 7): every step of the loop converges at the round's
                       first check and is carried into the next step inside the round;
    second_12_4_30     the same under strong process noise at a tighter tolerance: steps that need a second round (CONTINUE at the first check);
    absent_12_4_29,    trailing stages absent: the owner lanes of wave 7 are dead (31-stage schedule, the (12,4) instantiation as above);
    absent_12_4_28
    trailing_12_4_21   22 stages on the 31-stage schedule: waves 6 and 7 own absent stages only, two top rows multiply zeros;
    unfused_12_4_20    the 21-stage schedule, NOT fused: six groups of stages on eight waves -- waves 6 and 7 own none -- NTOP = 5 (an odd number of
                       column pairs), the top called straight from latw_solve;
    short_12_4_10      the 11-stage schedule: NTOP = 2, fewer column pairs than the four accumulator chains -- the chains are summed one after the
                       other, not in pairs;
    refactor_12_4_30   run COLD (no solve at setup) at eps 1e-9: the launch's first solve estimates rho and refactors inside the launch, which
                       rewrites the top inverse in LDS between two rounds -- no value fetched before may outlive that."""
import os

import numpy as np

from util import GOLDEN_DIR, stacked_batch, forced

PREFETCH_DIR = os.path.join(GOLDEN_DIR, 'latw_top_prefetch')
BATCH = 3
STEPS = 6
CHK = 25                    # OSQP's check interval: the round's own first test runs at iteration 25
SOLVED = 1

# name -> (nx, nu, Np, mode in the kernel's name, eps_abs = eps_rel, standard deviation of the process noise, cold)
CASES = {
    'first_12_4_30': (12, 4, 30, 231, 1e-1, 0.002, False),         # (a loose tolerance: what ends every solve at iteration 25)
    'second_12_4_30': (12, 4, 30, 231, 1e-4, 0.3, False),
    'absent_12_4_29': (12, 4, 29, 231, 1e-4, 0.3, False),
    'absent_12_4_28': (12, 4, 28, 231, 1e-4, 0.3, False),
    'trailing_12_4_21': (12, 4, 21, 231, 1e-4, 0.3, False),
    'unfused_12_4_20': (12, 4, 20, 221, 1e-4, 0.3, False),
    'short_12_4_10': (12, 4, 10, 211, 1e-4, 0.3, False),
    'refactor_12_4_30': (12, 4, 30, 231, 1e-9, 0.3, True),
}
KEYS = ('x', 'u', 'status', 'iter')


def kernel_suffix(name):
    nx, nu, Np, mode = CASES[name][:4]
    return ',%d,%d,%d,true>' % (((nx, nu) if mode == 231 else (0, 0)) + (mode,))      # (the (12,4) instantiation exists for the 31-stage schedule alone)


def compute(name):
    """(arrays, kernel name) of one case: x, u (float64), status, iter (int64) of the loop, and from the handle what the case is there for --
    carried: steps the round carried into the next step itself; refactorizations, checks: counters of mpcqp_get_stats over the launch alone."""
    from pympc_amd import fixtures
    nx, nu, Np, mode, eps, noise, cold = CASES[name]
    kws = [fixtures.random_lti(8100 + 17 * Np + i, nx=nx, nu=nu, Np=Np, xbox=10.0) for i in range(BATCH)]
    w = np.stack([noise * fixtures.random_lti_noise_rng(8100 + i).standard_normal((STEPS, nx)) for i in range(BATCH)], axis=1)
    with forced(backend='bcr8'):
        K = stacked_batch(kws, Nc=None, eps_feas=1e6, max_iter=4000, eps_abs=eps, eps_rel=eps)
        K.setup(solve=not cold)
    kn = K.prob.kernel_name(loop=True)
    K.prob.stats(reset=True)
    r = K.run(STEPS, w=w)
    st = K.prob.stats()
    out = {k: np.array(r[k], dtype=np.float64 if k in ('x', 'u') else np.int64) for k in KEYS}
    out['carried'] = np.array(K.prob.carry_stats()[0], dtype=np.int64)
    out['checks'] = np.array(st[1], dtype=np.int64)
    out['refactorizations'] = np.array(st[2], dtype=np.int64)
    return out, kn


def assert_precondition(name, g, kn):
    """What the recorded (or the repeated) run g of case `name` must show so that it is the path the case is about."""
    nx, nu, Np, mode, eps, noise, cold = CASES[name]
    assert kn.startswith('w8::k_mpc_run<16,') and kn.endswith(kernel_suffix(name)), (name, kn)
    st, it = g['status'], g['iter']
    assert st.shape == (STEPS, BATCH) and g['x'].shape == (STEPS + 1, BATCH, nx) and g['u'].shape == (STEPS, BATCH, nu), (name, st.shape)
    assert np.isfinite(g['x']).all() and np.isfinite(g['u']).all() and (it > 0).all(), name
    assert (st == SOLVED).all(), (name, st)
    assert int(g['carried']) > 0, (name, int(g['carried']))
    if name == 'refactor_12_4_30':
        assert int(g['refactorizations']) >= 1, (name, int(g['refactorizations']))
        return
    assert int(g['refactorizations']) == 0, (name, int(g['refactorizations']))
    if name == 'first_12_4_30':          # every solve of the loop ends at the round's first check (step 0 was solved by setup: the loop's first output)
        assert (it[1:] == CHK).all(), (name, it)
    if name == 'second_12_4_30':         # a CONTINUE at the first check, solved at a later one of the round's own
        assert ((it[1:] > CHK) & (it[1:] % CHK == 0) & (it[1:] % 100 != 0)).any(), (name, it)


def path(name):
    return os.path.join(PREFETCH_DIR, name + '.npz')
