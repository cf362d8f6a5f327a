"""Case table of tests/test_gpu_latw_boundary_bits.py, tests/test_latw_boundary_cases.py and scripts/record_latw_boundary_bits.py: the round
boundary of the latency round (latw_check and latw_carry, pympc_amd/csrc/mpcqp_latw_check.h) under weights the other goldens do not feed it.
P x of a lane is one dot product over Qx / QxN columns (state lanes) or over Qu / QDu entries of the own, the next and the previous stage (input
lanes); with the benchmark's diagonal weights most of its terms are zeros.  Here every weight matrix is dense and symmetric, QxN differs from
Qx, and the closed loops run under process noise at a tolerance at which solves need more than one check.

Shapes: (12,4,30), the specialised latw_check<12,4,31>; (4,2,21) and (3,1,30), the generic <0,0,21> and <0,0,31> -- absent trailing stages, and
nu = 1, where the previous and the next input of every input lie in another stage.  Each shape soft and hard; per case a batch of three:
    0      a plain instance under strong process noise: solves that cross a CONTINUE boundary, steps carried inside the round, and the item's
           last step, solved and not carried;
    1      a NaN disturbance into step NAN_STEP: the bounds of stage 0's dynamics rows stop being finite, their type changes, and the carry
           that made the transition hands the step back to begin (latw_carry returns LATW_SOLVED);
    2      soft: a NaN input reference -- q, every iterate and the objective are NaN, the check leaves on a non-finite residual (LATW_GENERIC);
           hard: a start far outside the state box -- primal infeasible, the certificate's cheap half sends the round to the generic check.
soft_12_4_30 runs its plant on caller-supplied matrices Ap / Bp (the carry's plant product from memory instead of the model's LDS copy).

Nc < Np: no case.  The cyclic-reduction backends refuse a held input (pympc_amd/csrc/mpcqp_plan.h, bcr_shape: !L.border; tests/util.py
bcr_schedule), so a controller forced to bcr8 with Nc < Np is not created and latw_check never sees Nc != Np.

assert_classes() states the exits as conditions on a recorded run: checked when the goldens are recorded, and again on the CPU over the files."""
import os

import numpy as np

from util import GOLDEN_DIR, stacked_batch, forced

BOUNDARY_DIR = os.path.join(GOLDEN_DIR, 'latw_boundary')
BATCH = 3
STEPS = 7                   # closed-loop steps, in one mpc_run
NOISE = 0.3                 # standard deviation of the process noise
NAN_STEP = 3                # instance 1's disturbance of this step is NaN in its first component
OUTSIDE = 40.0              # hard cases: instance 2 starts at OUTSIDE * XBOX in its first state
XBOX = 10.0
EPS = 1e-4                  # eps_abs = eps_rel: tight enough that warm-started solves under NOISE need a second check
CHK, RHO_EVERY = 25, 100    # OSQP's defaults: the round's own test runs at every multiple of CHK that is no multiple of RHO_EVERY
SOLVED, PRIMAL_INFEASIBLE = 1, -3

# name -> (nx, nu, Np, hard state box, caller-supplied plant)
CASES = {
    'soft_12_4_30': (12, 4, 30, False, True),
    'hard_12_4_30': (12, 4, 30, True, False),
    'soft_4_2_21': (4, 2, 21, False, False),
    'hard_4_2_21': (4, 2, 21, True, False),
    'soft_3_1_30': (3, 1, 30, False, False),
    'hard_3_1_30': (3, 1, 30, True, False),
}
FLOAT_KEYS = ('x', 'u', 'it_x', 'it_z', 'it_y', 'obj_val', 'pri_res', 'dua_res')
INT_KEYS = ('status', 'iter', 'info_status', 'info_iter', 'carried', 'handed_back')


def kernel_suffix(name):
    nx, nu, Np = CASES[name][:3]
    return ',%d,%d,231,true>' % ((12, 4) if (nx, nu) == (12, 4) else (0, 0))


def dense_spd(rng, n, scale):
    """scale * (I + M M' / (2 n)), M ~ N(0, 1): symmetric positive definite, every off-diagonal entry non-zero."""
    M = rng.standard_normal((n, n))
    S = M @ M.T
    return scale * (np.eye(n) + (S + S.T) / (4.0 * n))


def inputs(name):
    """(instance kwargs, disturbance [STEPS, BATCH, nx], plant (Ap, Bp) or (None, None)) of one case."""
    from pympc_amd import fixtures
    nx, nu, Np, hard, own_plant = CASES[name]
    kws = [fixtures.random_lti(7300 + 17 * nx + i, nx=nx, nu=nu, Np=Np, xbox=XBOX) for i in range(BATCH)]
    for i, kw in enumerate(kws):
        rng = np.random.default_rng(7300 + 100 * nx + i)
        kw.update(Qx=dense_spd(rng, nx, 1.0), QxN=dense_spd(rng, nx, 3.0), Qu=dense_spd(rng, nu, 0.1), QDu=dense_spd(rng, nu, 0.2))
    w = np.stack([NOISE * fixtures.random_lti_noise_rng(7300 + i).standard_normal((STEPS, nx)) for i in range(BATCH)], axis=1)
    w[:, 2] *= 0.03
    w[NAN_STEP, 1, 0] = np.nan
    if hard:
        kws[2]['x0'] = kws[2]['x0'].copy()
        kws[2]['x0'][0] = OUTSIDE * XBOX
    else:
        kws[2]['uref'] = np.full(nu, np.nan)
    Ap = Bp = None
    if own_plant:
        rng = np.random.default_rng(7399)
        Ap = np.stack([kw['Ad'] * (1.0 + 0.05 * rng.standard_normal((nx, nx))) for kw in kws])
        Bp = np.stack([kw['Bd'] * (1.0 + 0.05 * rng.standard_normal((nx, nu))) for kw in kws])
    return kws, w, (Ap, Bp)


def compute(name):
    """The arrays of one case and the kernel's name: x, u, status, iter of STEPS closed-loop steps, the stored iterate, the last record."""
    import warnings
    nx, nu, Np, hard, own_plant = CASES[name]
    kws, w, (Ap, Bp) = inputs(name)
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                   # (an infeasible or non-finite solve warns: it is what the instance is there for)
        with forced(backend='bcr8'):
            K = stacked_batch(kws, Nc=None, eps_feas=1e6, SOFT_ON=not hard, max_iter=2000, eps_abs=EPS, eps_rel=EPS)
            K.setup()
        kn = K.prob.kernel_name(loop=True)
        r = K.run(STEPS, w=w, Ap=Ap, Bp=Bp)
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
    """How often each exit of the boundary occurs in the recorded run g of case `name`, counted over the loop's own solves (step 0 is setup's)."""
    nx, nu, Np, hard, own_plant = CASES[name]
    st, it, x = g['status'], g['iter'], g['x']
    assert st.shape == (STEPS, BATCH) and x.shape == (STEPS + 1, BATCH, nx), (st.shape, x.shape)
    assert (st[:, 0] == SOLVED).all() and np.isfinite(x[:, 0]).all(), (name, st)
    loop_solved = (st[1:] == SOLVED) & own_check(it[1:])                     # solved at one of the round's own checks
    c = dict(carried=int(g['carried']), handed_back=int(g['handed_back']))
    # the run's last step has no next step to be carried into: solved at one of the round's own checks, it left through LATW_SOLVED
    c['solved_not_carried'] = int(loop_solved[-1].sum())
    c['continue'] = int(((st[1:, 0] == SOLVED) & own_check(it[1:, 0]) & (it[1:, 0] > CHK)).sum())      # LATW_CONTINUE at the first check, solved at a later one
    assert np.isfinite(x[:NAN_STEP + 1, 1]).all() and np.isnan(x[NAN_STEP + 1:, 1]).any(axis=1).all(), (name, x[:, 1])
    if hard:      # outside a hard box: primal infeasible, found at one of the round's own checks -- LATW_GENERIC on the certificate's cheap half
        c['generic'] = int((x[0, 2, 0] > XBOX) * ((st[1:, 2] == PRIMAL_INFEASIBLE) & own_check(it[1:, 2])).sum())
    else:         # a NaN objective: the round's own test leaves for the generic check, which reports an unsolved step
        c['generic'] = int(((st[1:, 2] != SOLVED) & own_check(it[1:, 2])).sum())
    return c


def assert_classes(golden):
    """Every exit of the boundary occurs in the recorded runs {name: arrays} (a condition on the case table, not a measurement), in EVERY case:
    a carried step, a solve that ended solved without being carried, a CONTINUE, a transition handed back to begin, and LATW_GENERIC."""
    cs = {name: classes(name, golden[name]) for name in CASES}
    for name, c in cs.items():
        assert c['carried'] > 0 and c['solved_not_carried'] > 0 and c['continue'] > 0 and c['handed_back'] > 0 and c['generic'] > 0, (name, c)
    return cs


def path(name):
    return os.path.join(BOUNDARY_DIR, name + '.npz')
