"""Named closed loops for the taped rollout and its reverse sweep (tests/test_rollout_cases.py pins the table on the CPU oracle,
tests/test_gpu_rollout.py holds the device to the restatement tests/rollout_ref.py on it).

Every instance is  fixtures.random_lti(7200 + seed, nx, nu, Np, xbox, ubox=0.5, dubox=0.25), x0 scaled by the case's factor,  stepped K times with plant = model and no
disturbance, at eps 1e-9.  For every listed (case, seed) every step ends 'solved', no step has a weakly active row even at 1000 times the
device's weak_tol, at least one step has two or more active inequality rows, one pair of consecutive solves has equal active sets and one
pair has different ones -- over the K + 1 solves of the K steps, the one for x_K included (K = 2 has two pairs that way).
tests/test_rollout_cases.py asserts all of it: a seed that fails is replaced here, not tolerated there.
"""
import numpy as np

import util

SEED_BASE = 7200

# name -> shape, SOFT_ON, state box, factor on x0, steps, seeds, reference rows (1: constant, 0: Np + 1 rows), the path it is there for
CASES = {
    'first':       dict(nx=4,  nu=2, Np=10,  Nc=10,  soft=True,  xbox=4.0, scale=1.0, K=6, seeds=(0, 3, 4, 5, 6), tv=False, path='NB 16, the loop settles: factor reuse'),
    'first_tvref': dict(nx=4,  nu=2, Np=10,  Nc=10,  soft=True,  xbox=4.0, scale=1.0, K=6, seeds=(0, 3, 6), tv=True,  path='time-varying reference, Np + 1 rows'),
    'headline':    dict(nx=12, nu=4, Np=30,  Nc=30,  soft=True,  xbox=4.0, scale=1.0, K=3, seeds=(0, 2, 11), tv=False, path="the headline backend's shape"),
    'nb32_soft':   dict(nx=20, nu=5, Np=6,   Nc=6,   soft=True,  xbox=4.0, scale=1.0, K=3, seeds=(4, 8, 24), tv=False, path='NB 32 with slack variables'),
    'held':        dict(nx=5,  nu=3, Np=12,  Nc=6,   soft=True,  xbox=4.0, scale=1.0, K=4, seeds=(3, 5, 7), tv=False, path='held input (border), Nc < Np'),
    'hard':        dict(nx=7,  nu=7, Np=4,   Nc=4,   soft=False, xbox=4.0, scale=1.0, K=4, seeds=(5, 7, 8), tv=False, path='no slack columns'),
    'long':        dict(nx=4,  nu=2, Np=100, Nc=100, soft=True,  xbox=4.0, scale=1.0, K=3, seeds=(3, 4), tv=False, path='long horizon'),
    'nb128':       dict(nx=64, nu=5, Np=3,   Nc=3,   soft=True,  xbox=4.0, scale=0.85, K=2, seeds=(42, 78), tv=False, path='NB 128 (huge layout)'),
    'nb64':        dict(nx=36, nu=6, Np=4,   Nc=4,   soft=True,  xbox=4.0, scale=0.7, K=2, seeds=(11, 42, 57), tv=False, path='NB 64 (wide layout)'),
}
FIRST = 'first'
WEAK_FACTOR = 1000.0       # the weak-row margin of the table, in units of the device's weak_tol


def pairs():
    """Every (case, seed) of the table."""
    return [(name, s) for name, c in CASES.items() for s in c['seeds']]


def draw(name, seed):
    """(constructor kwargs of MPCController, attributes to set afterwards) of one instance."""
    from pympc_amd import fixtures
    c = CASES[name]
    kw = dict(fixtures.random_lti(SEED_BASE + seed, nx=c['nx'], nu=c['nu'], Np=c['Np'], xbox=c['xbox'], ubox=0.5, dubox=0.25))
    kw['x0'] = kw['x0'] * c['scale']
    if c['Nc'] != c['Np']:
        kw['Nc'] = c['Nc']
    if c['tv']:                                            # a reference that moves along the horizon: Np + 1 rows
        r = np.random.RandomState(SEED_BASE + seed)
        kw['xref'] = np.asarray(kw['xref'], dtype=float)[None, :] + 0.05 * r.randn(c['Np'] + 1, c['nx'])
    return kw, ({} if c['soft'] else {'SOFT_ON': False})


def xref_traj(name, seed):
    """The references of steps 1 .. K of a time-varying case [K, Np + 1, nx] (entry k - 1 is what the solve after step k - 1 uses), else None."""
    c = CASES[name]
    if not c['tv']:
        return None
    kw, _ = draw(name, seed)
    r = np.random.RandomState(SEED_BASE + seed + 50)
    return np.asarray(kw['xref'], dtype=float)[None] + 0.02 * r.randn(c['K'], c['Np'] + 1, c['nx'])


def batch_kwargs(name, seeds=None, **settings):
    """BatchMPCController kwargs with the case's seeds (or the given ones) as its instances."""
    c = CASES[name]
    kws = [draw(name, s)[0] for s in (c['seeds'] if seeds is None else seeds)]
    return util.stacked(kws, Nc=c['Nc'], eps_feas=kws[0]['eps_feas'], SOFT_ON=c['soft'], **settings)


def oracle_controller(kw, attrs, eps=1e-9):
    """An MPCController on the CPU oracle (oracle/osqp_oracle.py), set up and cold-solved at eps_abs = eps_rel = eps."""
    return util.oracle_controller(kw, attrs, eps=eps, setup=True, quiet=True, max_iter=4000000)


def oracle_rollout(kw, attrs, K, Ap=None, Bp=None, w=None, xrefs=None, eps=1e-9, with_last=False):
    """Step the closed loop K times on the oracle: (tape, X [K+1, nx], U [K, nu], (D, E, c)).  The tape is in the form tests/rollout_ref.py
    takes; plant None: the controller's model; xrefs [K, ...]: the reference of the solve after step k; with_last: the solve for x_K, which
    is not on a tape, as entry K behind the others."""
    import warnings
    C = oracle_controller(kw, attrs, eps)
    nx, nu = np.asarray(kw['Bd']).shape
    A_p = np.asarray(kw['Ad'], dtype=float) if Ap is None else np.asarray(Ap, dtype=float)
    B_p = np.asarray(kw['Bd'], dtype=float) if Bp is None else np.asarray(Bp, dtype=float)
    x = np.array(kw['x0'], dtype=float)
    um1 = np.array(kw['uminus1'] if kw.get('uminus1') is not None else kw['uref'], dtype=float)
    xref = np.array(kw['xref'], dtype=float)
    tape, X, U = [], [x.copy()], []
    D, E, c = C.prob.scaling()
    for k in range(K):
        xi, zi, yi, _ = C.prob.iterate_state()
        solved = C.res.info.status == 'solved'
        tape.append(dict(x=xi.copy(), z=zi.copy(), y=yi.copy(), x0=x.copy(), um1=um1.copy(), xref=xref.copy(), solved=solved))
        u = np.array(C.output(), dtype=float).reshape(nu)
        x = A_p @ x + B_p @ u + (0.0 if w is None else np.asarray(w[k], dtype=float))
        um1 = u
        if xrefs is not None:
            xref = np.array(xrefs[k], dtype=float)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            C.update(x, u, xref=xref if xrefs is not None else None)
        X.append(x.copy()); U.append(u.copy())
    if with_last:
        xi, zi, yi, _ = C.prob.iterate_state()
        tape.append(dict(x=xi.copy(), z=zi.copy(), y=yi.copy(), x0=x.copy(), um1=um1.copy(), xref=xref.copy(), solved=C.res.info.status == 'solved'))
    return tape, np.array(X), np.array(U), (D, E, c)


def tape_facts(kw, attrs, tape, scaling, weak_tol=1e-6):
    """What the table promises about a tape: dict(solved [K] bool, n_weak [K] at WEAK_FACTOR weak_tol, n_ineq [K] active inequality rows,
    same [len - 1] bool: entries k and k + 1 have equal active sets)."""
    import adjoint_ref
    import adjoint_model_ref
    import rollout_ref
    D, E, c = scaling
    sets, weak, ineq = [], [], []
    for e in tape:
        (P, _, A, l, u), _ = adjoint_model_ref.build(rollout_ref.entry_kwargs(kw, e), attrs)
        low, upp = adjoint_ref.active_rows(A, l, u, e['x'], e['z'], e['y'], D, E, c)
        eq = np.clip(l, -adjoint_ref.QP_INFTY, adjoint_ref.QP_INFTY) == np.clip(u, -adjoint_ref.QP_INFTY, adjoint_ref.QP_INFTY)
        sets.append((low, upp))
        weak.append(adjoint_ref.count_weak(l, u, e['z'], e['y'], WEAK_FACTOR * weak_tol))
        ineq.append(int(np.count_nonzero((low | upp) & ~eq)))
    same = [bool(np.array_equal(sets[k][0], sets[k + 1][0]) and np.array_equal(sets[k][1], sets[k + 1][1])) for k in range(len(tape) - 1)]
    return dict(solved=np.array([e['solved'] for e in tape]), n_weak=np.array(weak), n_ineq=np.array(ineq), same=np.array(same, dtype=bool))
