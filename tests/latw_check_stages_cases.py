"""Case table of tests/test_gpu_latw_check_stages.py and of scripts/record_latw_check_stages.py: every way out of the latency round's own termination
test (latw_check, pympc_amd/csrc/mpcqp_latw_check.h), which reduces what a verdict 'solved' needs in a first stage and the cheap halves of the two
infeasibility certificates in a second one that only an unconverged solve reaches.  Closed loops on the device, shapes served by the generic
instantiation of the 31-stage schedule, soft and hard state boxes; per case a batch of five:
    0, 1   plain instances under strong and under weak process noise: solves that end at their second check and at their first, and steps
           carried inside the round;
    2      a NaN disturbance into step NAN_STEP.  It never reaches a residual: the bounds of stage 0's dynamics rows stop being finite, the rows
           stop being equalities, the carry that made the transition hands the step back (latw_carry returns LATW_SOLVED) and the solves go on
           finite with those rows free, beside a plant state that stays NaN;
    3      starts far outside its state box.  Hard box: stage 0's state is fixed outside it, the QP is primal infeasible, and the cheap half of that
           certificate sends the round to the generic check, which reports it.  Soft box: feasible through its slack, a long solve;
    4      a NaN input reference: q, and with it every iterate and the objective, is NaN in every solve -- the exit on a non-finite residual.
The inputs were chosen on the CPU oracle (oracle/osqp_oracle.py stepping the same loops), so that every class is non-empty there; assert_classes()
states the classes as conditions on a recorded run."""
import os

import numpy as np

from util import GOLDEN_DIR, stacked_batch, forced

STAGES_DIR = os.path.join(GOLDEN_DIR, 'latw_check_stages')
BATCH = 5
STEPS = 8                   # closed-loop steps, in one mpc_run
NOISE = 0.3                 # standard deviation of the process noise: large enough that some steps need a second check
NAN_STEP = 3                # instance 2's disturbance of this step is NaN in its first component
OUTSIDE = {False: 1.5, True: 40.0}      # instance 3 starts at OUTSIDE[hard] * xbox in its first state: a hard box stays violated for the whole run
XBOX = 10.0
CHK, RHO_EVERY = 25, 100    # OSQP's defaults: the round's own test runs at every multiple of CHK that is no multiple of RHO_EVERY
PRIMAL_INFEASIBLE = -3

# name -> (nx, nu, Np, hard state box, mode in the kernel's name)
CASES = {
    'soft_4_2_21': (4, 2, 21, False, 231),        # 22 stages: waves 6 and 7 own absent stages only
    'hard_4_2_21': (4, 2, 21, True, 231),
    'soft_3_1_30': (3, 1, 30, False, 231),        # every stage present, four of sixteen owner lanes alive
    'hard_3_1_30': (3, 1, 30, True, 231),
}
FLOAT_KEYS = ('x', 'u', 'it_x', 'it_z', 'it_y', 'obj_val', 'pri_res', 'dua_res')
INT_KEYS = ('status', 'iter', 'info_status', 'info_iter', 'carried', 'handed_back')


def inputs(name):
    """(instance kwargs, disturbance [STEPS, BATCH, nx]) of one case."""
    from pympc_amd import fixtures
    nx, nu, Np, hard, mode = CASES[name]
    kws = [fixtures.random_lti(6100 + 13 * nx + i, nx=nx, nu=nu, Np=Np, xbox=XBOX) for i in range(BATCH)]
    kws[3]['x0'] = kws[3]['x0'].copy()
    kws[3]['x0'][0] = OUTSIDE[hard] * XBOX
    w = np.stack([NOISE * fixtures.random_lti_noise_rng(6100 + i).standard_normal((STEPS, nx)) for i in range(BATCH)], axis=1)
    w[:, 1] *= 0.03                                       # (instance 1 barely moves: warm starts that converge at the first check)
    w[:, 3] *= 0.03
    w[NAN_STEP, 2, 0] = np.nan
    kws[4]['uref'] = np.full(nu, np.nan)
    return kws, w


def compute(name):
    """The arrays of one case and the kernel's name: x, u, status, iter of STEPS closed-loop steps, the stored iterate, the last record."""
    import warnings
    nx, nu, Np, hard, mode = CASES[name]
    kws, w = inputs(name)
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                   # (an infeasible solve warns: it is what the case is about)
        with forced(backend='bcr8'):
            K = stacked_batch(kws, Nc=None, eps_feas=1e6, SOFT_ON=not hard, max_iter=2000)
            K.setup()
        kn = K.prob.kernel_name(loop=True)
        r = K.run(STEPS, w=w)
    for k in ('x', 'u'):
        out[k] = np.array(r[k], dtype=np.float64)
    for k in ('status', 'iter'):
        out[k] = np.array(r[k], dtype=np.int64)
    for tag, v in zip('xzy', K.prob.iterate_state()):
        out['it_' + tag] = np.array(v, dtype=np.float64)
    infos = K.prob.infos()
    for k in ('obj_val', 'pri_res', 'dua_res'):
        out[k] = np.array([getattr(i, k) for i in infos], dtype=np.float64)
    out['info_status'] = np.array([i.status for i in infos], dtype=np.int64)
    out['info_iter'] = np.array([i.iter for i in infos], dtype=np.int64)
    out['carried'], out['handed_back'] = (np.array(v, dtype=np.int64) for v in K.prob.carry_stats()[:2])
    return out, kn


def own_check(it):
    """Iteration counts at which a solve can only have ended in the round's own test."""
    return (it > 0) & (it % CHK == 0) & (it % RHO_EVERY != 0)


def classes(name, g):
    """How often each exit of the check occurs in the recorded run g of case `name`, counted over the loop's own solves (step 0 is setup's)."""
    nx, nu, Np, hard, mode = CASES[name]
    st, it, x = g['status'], g['iter'], g['x']
    assert st.shape == (STEPS, BATCH) and x.shape == (STEPS + 1, BATCH, nx), (st.shape, x.shape)
    assert (st[1:, :2] == 1).all() and np.isfinite(x[:, [0, 1, 3]]).all(), (name, st)
    c = dict(first=int((it[1:, :2] == CHK).sum()),        # LATW_SOLVED / LATW_CARRIED at the solve's first check
             second=int((it[1:, :2] == 2 * CHK).sum()),   # LATW_CONTINUE, then solved
             carried=int(g['carried']))                   # LATW_CARRIED
    # the NaN disturbance of step NAN_STEP reaches the state of step NAN_STEP + 1: that transition is handed back
    assert np.isfinite(x[:NAN_STEP + 1, 2]).all() and np.isnan(x[NAN_STEP + 1:, 2]).any(axis=1).all(), (name, x[:, 2])
    c['handed_back'] = int(g['handed_back'])
    # a NaN objective: the round's own test leaves for the generic check, which reports an unsolved step
    c['nonfinite'] = int(((st[1:, 4] != 1) & own_check(it[1:, 4])).sum())
    # outside a hard box: primal infeasible, found at one of the round's own checks -- LATW_GENERIC on the certificate's cheap half
    c['certificate'] = int((hard and x[0, 3, 0] > XBOX) * ((st[1:, 3] == PRIMAL_INFEASIBLE) & own_check(it[1:, 3])).sum())
    return c


def assert_classes(golden):
    """Every exit of the check occurs in the recorded runs {name: arrays} (a condition on the case table, not a measurement): in every case a
    carried step, a transition handed back and the non-finite exit, under every hard box the certificate's, and over the table first-check and second-check solves."""
    cs = {name: classes(name, golden[name]) for name in CASES}
    for name, c in cs.items():
        assert c['carried'] > 0 and c['handed_back'] > 0 and c['nonfinite'] > 0 and c['second'] > 0, (name, c)
        assert c['certificate'] > 0 or not CASES[name][3], (name, c)
    assert sum(c['first'] for c in cs.values()) > 0, cs
    return cs


def path(name):
    return os.path.join(STAGES_DIR, name + '.npz')
