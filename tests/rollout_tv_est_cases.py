"""Named output-feedback loops under a model schedule for the taped rollout of include_ext2/mpcqp_rollout_tv_est.h and its reverse sweep
(tests/test_rollout_tv_est_cases.py pins the table on the CPU oracle, tests/test_gpu_rollout_tv_est.py holds the device to the restatement
tests/rollout_tv_est_ref.py on it).

Instance (case, seed, hold) is the controller of tests/rollout_cases.py under the schedule  rollout_tv_cases.schedule(case, seed, hold)  with
C, x_true0, v, w of  rollout_est_cases.estimator(case, seed)  and one gain per schedule entry,

    L_e = kalman_design_simple(Ad_traj[e], None, C, None, 0.01 I, 0.01 I, 'filter')[0]

the plant the entry in force, the estimate starting at the case's x0, holds 1 and 2.  The loop is mpcqp_mpc_loop_tv_est's: at a boundary step
the input of the last solve is applied, THEN the entry replaces the model; plant and estimator step under the entry in force with its gain
and the next solve is made under it.  For every (case, seed, hold) of the table, at eps 1e-9: all K + 1 solves end 'solved', no row is weakly
active at 1000 times the device's weak_tol, some step has two or more active inequality rows, and consecutive solves show both equal and
different active sets.  tests/test_rollout_tv_est_cases.py asserts all of it: a seed that fails is replaced here, not tolerated there.
('headline' / 2 has a weak row at step 1 on this loop and is left out.)
"""
import warnings

import numpy as np

import rollout_cases as rc
import rollout_est_cases as ec
import rollout_tv_cases as tc

NAMES = ('first', 'held', 'hard', 'headline', 'nb32_soft')
HOLDS = (1, 2)
SEEDS = {
    'first': (0, 3, 4, 6),
    'held': (3, 5, 7),
    'hard': (5, 7, 8),
    'headline': (0, 11),
    'nb32_soft': (4, 8, 24),
}
FIRST = 'first'
NOISE = 0.01               # Qn = NOISE I, Rn = NOISE I of every gain


def triples():
    """Every (case, seed, hold) of the table."""
    return [(name, s, hold) for name in NAMES for s in SEEDS[name] for hold in HOLDS]


def gains(Adt, C):
    """L [nseg, nx, ny]: the stationary Kalman filter gain of every schedule entry."""
    from pympc_amd.kalman import kalman_design_simple
    C = np.asarray(C, dtype=float)
    ny, nx = C.shape
    return np.stack([kalman_design_simple(np.asarray(A, dtype=float), None, C, None, NOISE * np.eye(nx), NOISE * np.eye(ny), 'filter')[0] for A in Adt])


def instance(name, seed, hold):
    """dict(kw, attrs, K, Adt, Bdt, C, Lt [nseg, nx, ny], x_true0, v, w) of one (case, seed, hold)."""
    kw, attrs = rc.draw(name, seed)
    Adt, Bdt = tc.schedule(name, seed, hold)
    est = ec.estimator(name, seed)
    return dict(kw=kw, attrs=attrs, K=rc.CASES[name]['K'], Adt=Adt, Bdt=Bdt, C=est['C'], Lt=gains(Adt, est['C']), x_true0=est['x_true0'], v=est['v'], w=est['w'])


def batch_instance(name, hold, seeds=None):
    """The instances of a case stacked the way the device takes them: dict(Adt [nseg, B, nx, nx], Bdt, Lt [nseg, B, nx, ny], C [B, ny, nx],
    x_true0 [B, nx], v [K, B, ny], w [K, B, nx]) and ``each``, the list of the single instances."""
    each = [instance(name, s, hold) for s in (SEEDS[name] if seeds is None else seeds)]
    st = lambda key, axis: np.ascontiguousarray(np.stack([i[key] for i in each], axis=axis))
    return dict(Adt=st('Adt', 1), Bdt=st('Bdt', 1), Lt=st('Lt', 1), C=st('C', 0), x_true0=st('x_true0', 0), v=st('v', 1), w=st('w', 1), each=each)


def oracle_rollout(kw, attrs, K, Adt, Bdt, hold, C, Lt, x_true0, v=None, w=None, Ap=None, Bp=None, eps=1e-9, with_last=False):
    """Step the output-feedback loop under the schedule K times on the oracle, in the order of mpcqp_mpc_loop_tv_est:
    (tape, X [K+1, nx], XH [K+1, nx], Y [K, ny], U [K, nu], slots).  The tape is in the form tests/rollout_tv_est_ref.py takes, the slots in
    that of tests/rollout_tv_ref.py; plant None: the entry in force; the estimate starts at kw's x0."""
    Kc = rc.oracle_controller(kw, attrs, eps)
    nx, nu = np.asarray(kw['Bd']).shape
    C = np.asarray(C, dtype=float)
    x = np.array(x_true0, dtype=float)
    xh = np.array(kw['x0'], dtype=float)
    um1 = np.array(kw['uminus1'] if kw.get('uminus1') is not None else kw['uref'], dtype=float)
    xref = np.array(kw['xref'], dtype=float)
    D, E, c = Kc.prob.scaling()[:3]
    slots = [dict(Ad=np.array(kw['Ad'], dtype=float), Bd=np.array(kw['Bd'], dtype=float), D=D, E=E, c=c)]
    tape, X, XH, Y, U = [], [x.copy()], [xh.copy()], [], []

    def entry(y):
        xi, zi, yi, _ = Kc.prob.iterate_state()
        return dict(x=xi.copy(), z=zi.copy(), y=yi.copy(), x0=xh.copy(), um1=um1.copy(), xref=xref.copy(), solved=Kc.res.info.status == 'solved',
                    x_plant=x.copy(), y_meas=None if y is None else y.copy())
    for k in range(K):
        y = C @ x + (0.0 if v is None else np.asarray(v[k], dtype=float))
        tape.append(entry(y))
        u = np.array(Kc.output(), dtype=float).reshape(nu)
        e = k // hold
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            Ad, Bd, L = np.asarray(Adt[e], dtype=float), np.asarray(Bdt[e], dtype=float), np.asarray(Lt[e], dtype=float)
            if k % hold == 0:
                Kc.update_model(Ad=Ad.copy(), Bd=Bd.copy(), solve=False)
                D, E, c = Kc.prob.scaling()[:3]
                slots.append(dict(Ad=Ad.copy(), Bd=Bd.copy(), D=D, E=E, c=c))
            A_p = Ad if Ap is None else np.asarray(Ap, dtype=float)
            B_p = Bd if Bp is None else np.asarray(Bp, dtype=float)
            x = A_p @ x + B_p @ u + (0.0 if w is None else np.asarray(w[k], dtype=float))
            xh = Ad @ (xh + L @ (y - C @ xh)) + Bd @ u
            um1 = u
            Kc.update(xh, u)
        X.append(x.copy()); XH.append(xh.copy()); Y.append(y.copy()); U.append(u.copy())
    if with_last:
        tape.append(entry(None))
    return tape, np.array(X), np.array(XH), np.array(Y), np.array(U), slots
