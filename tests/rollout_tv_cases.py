"""Named closed loops under a model schedule for the taped rollout of include_ext/mpcqp_rollout_tv.h and its reverse sweep
(tests/test_rollout_tv_cases.py pins the table on the CPU oracle, tests/test_gpu_rollout_tv.py holds the device to the restatement
tests/rollout_tv_ref.py on it).

The instances are those of tests/rollout_cases.py -- the cases below with the seeds listed there -- and the schedule of instance
(case, seed) is  ltv_models.model_schedule(Ad, Bd, nseg, amp=0.03)  around its own model, nseg = ceil(K / hold), for hold 1 and 2.  The loop
is mpcqp_mpc_loop_tv's: at a boundary step the input of the last solve is applied, THEN the entry replaces the model (update_model keeps the
iterate), the plant steps under the entry in force and the next solve is made under it.  For every (case, seed, hold), at eps 1e-9: all
K + 1 solves end 'solved', no row is weakly active at 1000 times the device's weak_tol, some step has two or more active inequality rows,
and consecutive solves show both equal and different active sets.  tests/test_rollout_tv_cases.py asserts all of it: a seed that fails is
replaced here, not tolerated there.
"""
import warnings

import numpy as np

import rollout_cases as rc
from ltv_models import model_schedule

NAMES = ('first', 'headline', 'held', 'hard', 'nb32_soft')
HOLDS = (1, 2)
AMP = 0.03
# (case -> seeds; the listed seeds of tests/rollout_cases.py)
SEEDS = {name: rc.CASES[name]['seeds'] for name in NAMES}


def nseg(name, hold):
    K = rc.CASES[name]['K']
    return (K + hold - 1) // hold


def triples():
    """Every (case, seed, hold) of the table."""
    return [(name, s, hold) for name in NAMES for s in SEEDS[name] for hold in HOLDS]


def schedule(name, seed, hold):
    """(Ad [nseg, nx, nx], Bd [nseg, nx, nu]) of one instance."""
    kw, _ = rc.draw(name, seed)
    return model_schedule(kw['Ad'], kw['Bd'], nseg(name, hold), amp=AMP)


def batch_schedule(name, hold, seeds=None):
    """(Ad [nseg, B, nx, nx], Bd [nseg, B, nx, nu]) of the case's instances."""
    sched = [schedule(name, s, hold) for s in (SEEDS[name] if seeds is None else seeds)]
    return np.stack([a for a, _ in sched], axis=1), np.stack([b for _, b in sched], axis=1)


def oracle_rollout(kw, attrs, K, Adt, Bdt, hold, Ap=None, Bp=None, w=None, eps=1e-9, with_last=False):
    """Step the closed loop under the schedule K times on the oracle, in the order of mpcqp_mpc_loop_tv: (tape, X [K+1, nx], U [K, nu], slots).
    The tape and the slots are in the form tests/rollout_tv_ref.py takes (slot 0: the model of kw; slot e + 1: entry e, with the scaling
    the oracle equilibrated it to); plant None: the entry in force; with_last: the solve for x_K as entry K behind the others."""
    C = rc.oracle_controller(kw, attrs, eps)
    nx, nu = np.asarray(kw['Bd']).shape
    x = np.array(kw['x0'], dtype=float)
    um1 = np.array(kw['uminus1'] if kw.get('uminus1') is not None else kw['uref'], dtype=float)
    xref = np.array(kw['xref'], dtype=float)
    D, E, c = C.prob.scaling()[:3]
    slots = [dict(Ad=np.array(kw['Ad'], dtype=float), Bd=np.array(kw['Bd'], dtype=float), D=D, E=E, c=c)]
    tape, X, U = [], [x.copy()], []

    def entry():
        xi, zi, yi, _ = C.prob.iterate_state()
        return dict(x=xi.copy(), z=zi.copy(), y=yi.copy(), x0=x.copy(), um1=um1.copy(), xref=xref.copy(), solved=C.res.info.status == 'solved')
    for k in range(K):
        tape.append(entry())
        u = np.array(C.output(), dtype=float).reshape(nu)
        e = k // hold
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            if k % hold == 0:
                C.update_model(Ad=np.array(Adt[e], dtype=float), Bd=np.array(Bdt[e], dtype=float), solve=False)
                D, E, c = C.prob.scaling()[:3]
                slots.append(dict(Ad=np.array(Adt[e], dtype=float), Bd=np.array(Bdt[e], dtype=float), D=D, E=E, c=c))
            A_p = np.asarray(Adt[e] if Ap is None else Ap, dtype=float)
            B_p = np.asarray(Bdt[e] if Bp is None else Bp, dtype=float)
            x = A_p @ x + B_p @ u + (0.0 if w is None else np.asarray(w[k], dtype=float))
            um1 = u
            C.update(x, u)
        X.append(x.copy()); U.append(u.copy())
    if with_last:
        tape.append(entry())
    return tape, np.array(X), np.array(U), slots


def tape_facts(kw, attrs, tape, slots, hold, weak_tol=1e-6):
    """rollout_cases.tape_facts with every entry under its own slot: dict(solved, n_weak, n_ineq [len], same [len - 1] bool, slot [len])."""
    import adjoint_ref
    import adjoint_model_ref
    import rollout_ref
    import rollout_tv_ref
    sets, weak, ineq, sl = [], [], [], []
    for k, e in enumerate(tape):
        s = slots[rollout_tv_ref.sigma(k, hold)]
        (P, _, A, l, u), _ = adjoint_model_ref.build(rollout_ref.entry_kwargs(rollout_tv_ref.with_slot(kw, s), e), attrs)
        low, upp = adjoint_ref.active_rows(A, l, u, e['x'], e['z'], e['y'], s['D'], s['E'], s['c'])
        eq = np.clip(l, -adjoint_ref.QP_INFTY, adjoint_ref.QP_INFTY) == np.clip(u, -adjoint_ref.QP_INFTY, adjoint_ref.QP_INFTY)
        sets.append((low, upp))
        weak.append(adjoint_ref.count_weak(l, u, e['z'], e['y'], rc.WEAK_FACTOR * weak_tol))
        ineq.append(int(np.count_nonzero((low | upp) & ~eq)))
        sl.append(rollout_tv_ref.sigma(k, hold))
    same = [bool(np.array_equal(sets[k][0], sets[k + 1][0]) and np.array_equal(sets[k][1], sets[k + 1][1])) for k in range(len(tape) - 1)]
    return dict(solved=np.array([e['solved'] for e in tape]), n_weak=np.array(weak), n_ineq=np.array(ineq), same=np.array(same, dtype=bool),
                slot=np.array(sl))
