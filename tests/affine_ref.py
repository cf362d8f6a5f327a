"""The CPU reference of the affine term in the prediction model, x_{k+1} = Ad x_k + Bd u_k + d_k (include_ext4/mpcqp_affine.h): the project's CPU
oracle (oracle/osqp_oracle.py) used as a general OSQP on the QP pympc_amd.qp_build makes, with l = u = 0.0 - d_k on the rows of stage k + 1.
tests/test_affine_ref.py pins it two independent ways; tests/test_gpu_affine.py holds the kernels to it.  Cases are those of
tests/settings_cases.py, so that every kernel family is met at its smallest shape.
"""
import warnings

import numpy as np

import settings_cases as sc

# the cases of the GPU tests and the scale s of their term, d = s max(1, |x0|_inf) N(0, 1): at these scales the oracle's tight solution has at
# least one active inequality row on every case (asserted in tests/test_affine_ref.py), so the term reaches the projections
SCALE = {'point_mass': 0.1, 'random_5_3_8': 0.1, 'quadcopter': 0.1, 'random_12_4_30_hard': 0.1, 'random_12_4_30_tight': 0.1, 'random_20_8_12_b': 0.1,
         'cart_pole_nc1': 0.02, 'group_3_2_50_20_tight': 0.1, 'group_5_3_40_40': 0.3, 'wide_25_8_3_tight': 0.1, 'wide_70_10_5_tight': 0.1}
ONE_ROW = ('point_mass', 'random_5_3_8', 'random_12_4_30_tight', 'random_20_8_12_b', 'cart_pole_nc1', 'group_3_2_50_20_tight', 'wide_25_8_3_tight',
           'wide_70_10_5_tight')          # one case per kernel family also runs with d_rows = 1
B = 3                                     # instances of a batch, each with a term of its own
TIGHT = 1e-9


def shape(case):
    kw, _ = sc.draw(case)
    nx = np.asarray(kw['Ad']).shape[0]
    return nx, np.asarray(kw['Bd'], dtype=float).reshape(nx, -1).shape[1], kw['Np']


def term(case, rows=None, batch=B, entries=None):
    """d [batch, rows, nx] (rows: Np, or 1) -- or, with ``entries``, a schedule [entries, batch, rows, nx] -- of a case: s max(1, |x0|_inf) N(0, 1)
    from default_rng(7)."""
    kw, _ = sc.draw(case)
    nx, _, Np = shape(case)
    rows = Np if rows is None else rows
    s = SCALE[case] * max(1.0, np.abs(np.asarray(kw['x0'], dtype=float)).max())
    lead = (batch,) if entries is None else (entries, batch)
    return s * np.random.default_rng(7).standard_normal(lead + (rows, nx))


def bounds(K, d):
    """(l, u) of controller K (set up) with the term d [nx], [1, nx] or [Np, nx] of ONE instance: copies of K.l, K.u with 0.0 - d_k on the rows
    of stage k + 1."""
    nx, Np = K.nx, K.Np
    l, u = np.array(K.l, dtype=float), np.array(K.u, dtype=float)
    rows = 0.0 - np.broadcast_to(np.asarray(d, dtype=float).reshape(-1, nx), (Np, nx)).ravel()
    l[nx:(Np + 1) * nx] = rows
    u[nx:(Np + 1) * nx] = rows
    return l, u


def put(K, d):
    """The term d of one instance into an ORACLE controller that is set up: its l, u and the oracle's."""
    l, u = bounds(K, d)
    K.l, K.u = l, u
    K.prob.update(l=l, u=u)


def oracle(case, d, eps=TIGHT, solve=True, x0=None, **more):
    """An oracle controller of the case, set up, with the term d of one instance in force; solved at eps (max_iter raised for a tight solve)."""
    if eps < 1e-6:
        more.setdefault('max_iter', 200000)
    K = sc.controller(case, 'default', True, eps=eps, x0=x0, **more)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K.setup(solve=False)
        put(K, d)
        if solve:
            K.solve()
    return K


_tight = {}


def tight(case, rows=None):
    """The oracle's tight solves of the B instances of a case (each with its own term): list of (x, y, status, l, u); made once."""
    key = (case, rows)
    if key not in _tight:
        out = []
        for d in term(case, rows):
            K = oracle(case, d)
            out.append((np.array(K.res.x), np.array(K.res.y), K.res.info.status, np.array(K.l), np.array(K.u)))
        _tight[key] = out
    return _tight[key]


def active_inequalities(case, x, l, u, tol=1e-7):
    """Inequality rows (l < u) of the case's QP on which A x sits on a bound."""
    K = sc.controller(case, 'default', True)
    K.setup(solve=False)
    z = K.A @ x
    ineq = u - l > 1e-9
    return int(np.sum(ineq & ((z - l < tol * np.maximum(1.0, np.abs(l))) | (u - z < tol * np.maximum(1.0, np.abs(u))))))


def u0_of(K):
    ou = (K.Np + 1) * K.nx
    return np.array(K.res.x[ou:ou + K.nu])


def plant(case):
    kw, _ = sc.draw(case)
    Ad = np.asarray(kw['Ad'], dtype=float)
    return Ad, np.asarray(kw['Bd'], dtype=float).reshape(Ad.shape[0], -1), np.asarray(kw['x0'], dtype=float)


# closed loops: STEPS steps of three instances, x0 scaled by the case's factors, each with its own term(s) and the disturbance sc.noise(nx).
# A factor is replaced like a seed (tests/settings_cases.py): at eps 1e-9 the stopping round of random_12_4_30_tight -- its soft state box is
# violated by O(1), a slack cost of 1e6 against weights of O(1) -- moves with the rounding of the KKT solve for the larger x0, and the ORACLE's
# own two elimination orders then give loops 1e-6 apart (instance 0 at factor 1.0: 125 against 225 iterations at step 1, factor 0.9: 1.0e-6).
# The listed factors are those on which the oracle's orders agree in every form, counts and all (tests/test_affine_ref.py asserts it).
LOOP_FACTORS = {'random_12_4_30_tight': (0.8, 0.7, 0.6)}
FORMS = ('constant', 'hold1', 'hold2_model')


def x0_factors(case):
    return LOOP_FACTORS.get(case, (1.0, 0.9, 0.6))


def schedule(case, form):
    """(d0 [B, Np, nx] or None, d_traj [entries, B, Np, nx] or None, hold, model_traj (Ad [entries, B, nx, nx], Bd, hold) or None) of a loop: a
    constant term; a schedule at hold = 1; a schedule at hold = 2 beside a model schedule of the same hold."""
    if form == 'constant':
        return term(case), None, 1, None
    if form == 'hold1':
        return None, term(case, entries=sc.STEPS), 1, None
    Ad, Bd, _ = plant(case)
    ne = (sc.STEPS + 1) // 2
    At = np.stack([np.stack([Ad * (1.0 - 0.02 * e)] * B) for e in range(ne)])
    Bt = np.stack([np.stack([Bd * (1.0 + 0.05 * e)] * B) for e in range(ne)])
    return None, term(case, entries=ne), 2, (At, Bt, 2)


def oracle_loop(case, copy, steps, w, d0, d_traj=None, hold=1, model_traj=None, model_hold=1, eps=TIGHT, iters=None, **more):
    """The closed loop of one instance stepped in Python on the oracle with the device loop's indexing: the first solve with the term d0 (None:
    none), the solve after step k with entry k // hold of d_traj [entries, rows, nx] (None: d0 throughout) under entry k // model_hold of
    model_traj = (Ad [entries, nx, nx], Bd [entries, nx, nu]) put in force at the start of step k.  The plant is the model in force WITHOUT the
    term, plus w[k].  Returns (x [steps + 1, nx], u [steps, nu], statuses); ``iters``: a list the iteration counts of the solves are appended to;
    ``more``: oracle settings (ordering=None: its other elimination order)."""
    Ad, Bd, x0 = plant(case)
    x = x0_factors(case)[copy] * x0
    K = sc.controller(case, 'default', True, eps=eps, x0=x.copy(), max_iter=200000, **more)
    iters = [] if iters is None else iters
    xs, us, st = [x.copy()], [], []
    zero = np.zeros(Ad.shape[0])
    d = zero if d0 is None else d0
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K.setup(solve=False)
        put(K, d)
        K.solve()
        iters.append(K.res.info.iter)
        for k in range(steps):
            u = np.array(K.output(), dtype=float).reshape(-1)
            if model_traj is not None and k % model_hold == 0:
                Ad, Bd = model_traj[0][k // model_hold], model_traj[1][k // model_hold]
                K.update_model(Ad=Ad, Bd=Bd, solve=False)      # (rebuilds l, u without the term: put back below)
                put(K, d)
            x = Ad @ x + Bd @ u + w[k]
            if d_traj is not None:
                d = d_traj[k // hold]
                put(K, d)
            K.update(x, u)
            xs.append(x.copy()); us.append(u); st.append(K.res.info.status); iters.append(K.res.info.iter)
    return np.array(xs), np.array(us), st


def state_of(K):
    """(P, q, A, l, u, x, z, y, D, E, c) of an oracle controller's last solve (unscaled), as tests/polish_ref.py and tests/adjoint_ref.py take it."""
    import scipy.sparse as sp
    x, z, y, _ = K.prob.iterate_state()
    D, E, c = K.prob.scaling()
    U = sp.triu(sp.csc_matrix(K.P), format='csc')
    P = (U + sp.triu(U, 1).T).tocsc()
    return P, np.asarray(K.q, dtype=float), sp.csc_matrix(K.A), np.asarray(K.l, dtype=float), np.asarray(K.u, dtype=float), x, z, y, D, E, c


# polish: x0 factors of random_12_4_30_tight's three instances on which OSQP's polish, restated on the CPU (tests/polish_ref.py), is ACCEPTED from the
# oracle's eps 1e-3 iterate and lands on the optimum (the tight solve, polished: equal to the last bit) while the unpolished u0 is 3e-5 .. 1e-4
# away -- the EXACT list of tests/test_gpu_polish.py, made the same way.  At factor 1.0 the eps 1e-3 iterate implies a wrong active set on all three
# and the polish is REJECTED (status -1): that batch is pinned too.  tests/test_affine_ref.py asserts both.
POLISH_FACTORS = (0.7, 0.6, 0.5)
_polished = {}


def polished(case, eps, factors=(1.0, 1.0, 1.0)):
    """Per instance of the case (term of Np rows, x0 scaled by its factor): the oracle's solve at eps polished on the CPU (tests/polish_ref.py) --
    (polished u0, status_polish, unpolished u0)."""
    import polish_ref
    key = (case, eps, tuple(factors))
    if key not in _polished:
        out = []
        x0 = plant(case)[2]
        for d, f in zip(term(case), factors):
            K = oracle(case, d, eps=eps, x0=f * x0)
            P, q, A, l, u, x, z, y, D, E, c = state_of(K)
            r = polish_ref.polish(P, q, A, l, u, x, z, y, D, E, c, K.res.info.pri_res, K.res.info.dua_res)
            ou = (K.Np + 1) * K.nx
            out.append((r['x'][ou:ou + K.nu], r['status_polish'], u0_of(K)))
        _polished[key] = out
    return _polished[key]
