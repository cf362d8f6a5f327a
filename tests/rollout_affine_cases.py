"""Named closed loops with an affine term in the prediction model for the taped rollout of include_ext5/mpcqp_rollout_affine.h and its reverse
sweep: the loops of tests/rollout_cases.py, each instance with a term d0 for its first solve and a schedule of terms behind it
(tests/test_rollout_affine_cases.py pins the table on the CPU oracle, tests/test_gpu_rollout_affine.py holds the device to the restatement
tests/rollout_affine_ref.py on it).

Every term is  SCALE max(1, |x0|_inf) N(0, 1)  from default_rng(7300 + seed) -- [K + 1, Np, nx], of which entry 0 is d0 and entries 1 .. the
schedule; a one-row term is stage 0 of it -- so the loops at rows = 1 and rows = Np, d_hold = 1 and 2 are four different loops.  For every listed
(case, seed) and every (rows, d_hold) every step ends 'solved', no step has a weakly active row at WEAK_FACTOR times the device's weak_tol, at
least one step has an active inequality row, one pair of consecutive solves has equal active sets and one pair has different ones.
tests/test_rollout_affine_cases.py asserts all of it: a seed that fails is replaced here, not tolerated there.
"""
import warnings

import numpy as np

import affine_ref
import util
import rollout_cases as rc

SCALE = 0.05
TERM_BASE = 7300
ROWS = ('1', 'Np')
HOLDS = (1, 2)
WEAK_FACTOR = rc.WEAK_FACTOR

# name -> seeds of tests/rollout_cases.draw that meet the conditions in all four (rows, d_hold).  (Replaced so far, each for a weakly active row or
# for active sets that never repeat or never change in one of the four: first 0, 3, 4, 5; held 3, 7; hard 7; headline 0, 2, 11; nb32_soft 4, 8.)
SEEDS = {
    'first': (6, 7),
    'held': (5, 1, 19),
    'hard': (5, 8),
    'headline': (6, 29),
    'nb32_soft': (24, 32),
}
NAMES = tuple(SEEDS)
SCHEDULED = ('first', 'held')          # the cases that also run under a model schedule (tests/rollout_tv_cases.py's, at its hold 2)


def combos():
    return [(rows, hold) for rows in ROWS for hold in HOLDS]


def triples():
    """Every (case, seed) of the table."""
    return [(name, s) for name in NAMES for s in SEEDS[name]]


def nrows(name, rows):
    return 1 if rows == '1' else rc.CASES[name]['Np']


def nent(name, hold):
    K = rc.CASES[name]['K']
    return (K + hold - 1) // hold


def terms(name, seed, rows, hold):
    """(d0 [rows, nx], d_traj [nent, rows, nx]) of one instance."""
    c = rc.CASES[name]
    kw, _ = rc.draw(name, seed)
    s = SCALE * max(1.0, np.abs(np.asarray(kw['x0'], dtype=float)).max())
    d = s * np.random.default_rng(TERM_BASE + seed).standard_normal((c['K'] + 1, c['Np'], c['nx']))
    d = d[:, :nrows(name, rows)]
    return d[0], d[1:1 + nent(name, hold)]


def batch_terms(name, rows, hold, seeds=None):
    """(d0 [B, rows, nx], d_traj [nent, B, rows, nx]) of the case's instances."""
    t = [terms(name, s, rows, hold) for s in (SEEDS[name] if seeds is None else seeds)]
    return np.stack([a for a, _ in t]), np.stack([b for _, b in t], axis=1)


def slots(d0, d_traj):
    """[nslots, rows, nx] of one instance: slot 0 the first solve's term, slot e + 1 schedule entry e."""
    return np.concatenate([np.asarray(d0, dtype=float)[None], np.asarray(d_traj, dtype=float)])


def oracle_rollout(kw, attrs, K, d0, d_traj, hold, w=None, eps=1e-9, with_last=False):
    """tests/rollout_cases.oracle_rollout with the term: the first solve under d0 (None: none), the solve after step k under entry k // hold of
    d_traj (None: d0 throughout), with the indexing of tests/affine_ref.oracle_loop -- ``put`` before ``update``.  The plant is the model without
    the term, plus w[k].  (tape, X, U, (D, E, c))."""
    C = util.oracle_controller(kw, attrs, eps=eps, setup=True, solve=False, quiet=True, max_iter=4000000)
    nx, nu = np.asarray(kw['Bd']).shape
    A_p, B_p = np.asarray(kw['Ad'], dtype=float), np.asarray(kw['Bd'], dtype=float)
    x = np.array(kw['x0'], dtype=float)
    um1 = np.array(kw['uminus1'] if kw.get('uminus1') is not None else kw['uref'], dtype=float)
    xref = np.array(kw['xref'], dtype=float)
    tape, X, U = [], [x.copy()], []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if d0 is not None:
            affine_ref.put(C, d0)
        C.solve()
        D, E, c = C.prob.scaling()

        def entry():
            xi, zi, yi, _ = C.prob.iterate_state()
            return dict(x=xi.copy(), z=zi.copy(), y=yi.copy(), x0=x.copy(), um1=um1.copy(), xref=xref.copy(), solved=C.res.info.status == 'solved')
        for k in range(K):
            tape.append(entry())
            u = np.array(C.output(), dtype=float).reshape(nu)
            x = A_p @ x + B_p @ u + (0.0 if w is None else np.asarray(w[k], dtype=float))
            um1 = u
            if d_traj is not None:
                affine_ref.put(C, d_traj[k // hold])
            C.update(x, u)
            X.append(x.copy()); U.append(u.copy())
        if with_last:
            tape.append(entry())
    return tape, np.array(X), np.array(U), (D, E, c)


def tape_facts(kw, attrs, tape, scaling, d_slots, hold, weak_tol=1e-6):
    """tests/rollout_cases.tape_facts with the term of slot tau(k) on entry k's dynamics rows."""
    import adjoint_ref
    import adjoint_model_ref
    import rollout_ref
    import rollout_affine_ref as ar
    D, E, c = scaling
    nx, Np = np.asarray(kw['Ad']).shape[0], kw['Np']
    sets, weak, ineq = [], [], []
    for k, e in enumerate(tape):
        (P, _, A, l, u), _ = adjoint_model_ref.build(rollout_ref.entry_kwargs(kw, e), attrs)
        l, u = ar.with_term(l, u, d_slots[ar.tau(k, hold)], nx, Np)
        low, upp = adjoint_ref.active_rows(A, l, u, e['x'], e['z'], e['y'], D, E, c)
        eq = np.clip(l, -adjoint_ref.QP_INFTY, adjoint_ref.QP_INFTY) == np.clip(u, -adjoint_ref.QP_INFTY, adjoint_ref.QP_INFTY)
        sets.append((low, upp))
        weak.append(adjoint_ref.count_weak(l, u, e['z'], e['y'], WEAK_FACTOR * weak_tol))
        ineq.append(int(np.count_nonzero((low | upp) & ~eq)))
    same = [bool(np.array_equal(sets[k][0], sets[k + 1][0]) and np.array_equal(sets[k][1], sets[k + 1][1])) for k in range(len(tape) - 1)]
    return dict(solved=np.array([e['solved'] for e in tape]), n_weak=np.array(weak), n_ineq=np.array(ineq), same=np.array(same, dtype=bool))
