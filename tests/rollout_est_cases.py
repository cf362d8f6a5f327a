"""Named output-feedback loops for the taped rollout through the estimator (include/mpcqp_rollout_est.h): tests/test_rollout_est_cases.py
pins the table on the CPU oracle, tests/test_gpu_rollout_est.py holds the device to the restatement tests/rollout_est_ref.py on it.

Every instance is a controller of tests/rollout_cases.py (the same shapes, plant = model, constant reference) with an estimator drawn by

    rng = np.random.default_rng(900 + seed)
    C = rng.standard_normal((ny, nx));  L = kalman_design_simple(Ad, None, C, None, 0.01 I, 0.01 I, 'filter')[0]
    x_true0 = x0 + 0.05 rng.standard_normal(nx);  v = 0.01 rng.standard_normal((K, ny));  w = 0.01 rng.standard_normal((K, nx))

in that order, ny = 2 for nx < 12 and 3 otherwise; the estimate starts at the case's x0.  For every listed (case, seed) the conditions of
tests/rollout_cases.py hold on the oracle's output-feedback loop at eps 1e-9: every step 'solved', no weak row at 1000 weak_tol, a step with
two or more active inequality rows, one equal and one different consecutive pair of active sets over the K + 1 solves.  A seed that stops
meeting them is replaced here, not tolerated in a test.  ('first' / 5 has a weak row at step 4 and is left out.)
"""
import numpy as np

import rollout_cases as rc

SEED_BASE = 900
SEEDS = {
    'first': (0, 3, 4, 6),
    'headline': (0, 2, 11),
    'nb32_soft': (4, 8, 24),
    'held': (3, 5, 7),
    'hard': (5, 7, 8),
    'long': (3, 4),
    'nb64': (11, 42, 57),
    'nb128': (42, 78),
}
FIRST = 'first'
REUSE_SEED = 3             # 'first' / 3: three factorizations over six entries (same = 0 0 1 1 1)
CASES = {name: dict(rc.CASES[name], seeds=SEEDS[name]) for name in SEEDS}


def pairs():
    return [(name, s) for name in SEEDS for s in SEEDS[name]]


def ny_of(name):
    return 2 if rc.CASES[name]['nx'] < 12 else 3


def estimator(name, seed):
    """dict(C [ny, nx], L [nx, ny], x_true0 [nx], v [K, ny], w [K, nx]) of one instance."""
    from pympc_amd.kalman import kalman_design_simple
    c = rc.CASES[name]
    kw, _ = rc.draw(name, seed)
    nx, K, ny = c['nx'], c['K'], ny_of(name)
    rng = np.random.default_rng(SEED_BASE + seed)
    C = rng.standard_normal((ny, nx))
    L = kalman_design_simple(kw['Ad'], None, C, None, 0.01 * np.eye(nx), 0.01 * np.eye(ny), 'filter')[0]
    x_true0 = np.asarray(kw['x0'], dtype=float) + 0.05 * rng.standard_normal(nx)
    v = 0.01 * rng.standard_normal((K, ny))
    w = 0.01 * rng.standard_normal((K, nx))
    return dict(C=C, L=L, x_true0=x_true0, v=v, w=w)


def batch_kwargs(name, seeds=None, **settings):
    return rc.batch_kwargs(name, SEEDS[name] if seeds is None else seeds, **settings)


def batch_estimator(name, seeds=None):
    """The estimators of a case's instances stacked: dict(C [B, ny, nx], L [B, nx, ny], x_true0 [B, nx], v [K, B, ny], w [K, B, nx])."""
    es = [estimator(name, s) for s in (SEEDS[name] if seeds is None else seeds)]
    return dict(C=np.stack([e['C'] for e in es]), L=np.stack([e['L'] for e in es]), x_true0=np.stack([e['x_true0'] for e in es]),
                v=np.stack([e['v'] for e in es], axis=1), w=np.stack([e['w'] for e in es], axis=1))


def oracle_rollout(kw, attrs, K, C, L, x_true0, v=None, w=None, Ap=None, Bp=None, eps=1e-9, with_last=False):
    """Step the output-feedback loop K times on the oracle: (tape, X [K+1, nx], XH [K+1, nx], Y [K, ny], U [K, nu], (D, E, c)).  The tape is
    in the form tests/rollout_est_ref.py takes: the entries of tests/rollout_ref.py (x0 = the estimate xh_k) with x_plant and y_meas beside."""
    import warnings
    Kc = rc.oracle_controller(kw, attrs, eps)
    nx, nu = np.asarray(kw['Bd']).shape
    Ad, Bd = np.asarray(kw['Ad'], dtype=float), np.asarray(kw['Bd'], dtype=float)
    A_p = Ad if Ap is None else np.asarray(Ap, dtype=float)
    B_p = Bd if Bp is None else np.asarray(Bp, dtype=float)
    C, L = np.asarray(C, dtype=float), np.asarray(L, dtype=float)
    x, xh = np.array(x_true0, dtype=float), np.array(kw['x0'], dtype=float)
    um1 = np.array(kw['uminus1'] if kw.get('uminus1') is not None else kw['uref'], dtype=float)
    xref = np.array(kw['xref'], dtype=float)
    tape, X, XH, Y, U = [], [x.copy()], [xh.copy()], [], []
    D, E, c = Kc.prob.scaling()

    def entry(y):
        xi, zi, yi, _ = Kc.prob.iterate_state()
        return dict(x=xi.copy(), z=zi.copy(), y=yi.copy(), x0=xh.copy(), um1=um1.copy(), xref=xref.copy(), solved=Kc.res.info.status == 'solved',
                    x_plant=x.copy(), y_meas=None if y is None else y.copy())
    for k in range(K):
        y = C @ x + (0.0 if v is None else np.asarray(v[k], dtype=float))
        tape.append(entry(y))
        u = np.array(Kc.output(), dtype=float).reshape(nu)
        x = A_p @ x + B_p @ u + (0.0 if w is None else np.asarray(w[k], dtype=float))
        xh = Ad @ (xh + L @ (y - C @ xh)) + Bd @ u
        um1 = u
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            Kc.update(xh, u)
        X.append(x.copy()); XH.append(xh.copy()); Y.append(y.copy()); U.append(u.copy())
    if with_last:
        tape.append(entry(None))
    return tape, np.array(X), np.array(XH), np.array(Y), np.array(U), (D, E, c)
