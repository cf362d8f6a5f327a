"""Restatement of the reverse sweep over a closed-loop rollout (include/mpcqp_rollout.h) for the tests: the recursion in numpy on top of
tests/adjoint_ref.py (the active-set KKT system by a sparse LU, the chain into x0, u_{-1}, xref, uref read off the host QP builder) and
tests/adjoint_model_ref.py (the model gradients as plain sums).  It shares nothing with the HIP kernel (pympc_amd/csrc/mpcqp_rollout.h).

One instance at a time.  A tape is a list of entries, entry k = dict(x [n], z [m], y [m] the iterate; x0 [nx], um1 [nu], xref [nx] or
[Np+1, nx] the step data its solve was made with; solved bool).  With G_x [K+1, nx] = dL/dx_k, G_u [K, nu] = dL/du_k and the plant
x_{k+1} = Ap x_k + Bp u_k + w_k (None: the controller's Ad, Bd), u_k the first input of entry k or uref where it is not solved:

    lam_K = G_x[K];  mu = 0
    for k = K-1 .. 0:
        g      = G_u[k] + Bp' lam_{k+1} + mu
        solved:      lam_k = G_x[k] + Ap' lam_{k+1} + d_x0(g);  mu = d_um1(g);  d_uref += d_uref(g);  d_xref[k] = d_xref(g);  model += model(g)
        not solved:  lam_k = G_x[k] + Ap' lam_{k+1};            mu = 0;         d_uref += g
        d_Ap  += lam_{k+1} x_k';   d_Bp += lam_{k+1} u_k'
    d_uminus1 = mu
"""
import numpy as np

import adjoint_ref
import adjoint_model_ref

MODEL_NAMES = adjoint_model_ref.NAMES


def entry_kwargs(kw, entry):
    """The controller's kwargs with the step data of a tape entry in place of x0, uminus1, xref."""
    k2 = adjoint_model_ref.full_kwargs(kw)
    k2['x0'], k2['uminus1'], k2['xref'] = np.array(entry['x0'], dtype=float), np.array(entry['um1'], dtype=float), np.array(entry['xref'], dtype=float)
    return k2


def sweep(kw, attrs, tape, D, E, c, G_x=None, G_u=None, Ap=None, Bp=None, weak_tol=adjoint_ref.WEAK_TOL, maps=None, cache=None):
    """Everything mpcqp_rollout_adjoint returns for one instance: dict lam [K+1, nx], uminus1, uref [nu], xref [K, p], Ap [nx, nx], Bp [nx, nu],
    the seven model gradients, n_active, n_weak, status [K], n_factor (1 + the changes of the active set along the solved entries, in sweep
    order), n_solved, and sets [K] (the (low, upp) masks of the solved entries, None elsewhere).  kw: constructor kwargs of MPCController;
    cache: a dict that keeps the QP of every entry between sweeps of one tape with different seeds."""
    attrs = attrs or {}
    K = len(tape)
    kwf = adjoint_model_ref.full_kwargs(kw)
    nx, nu = kwf['Bd'].shape
    Np = kwf['Np']
    ou = (Np + 1) * nx
    G_x = np.zeros((K + 1, nx)) if G_x is None else np.asarray(G_x, dtype=float)
    G_u = np.zeros((K, nu)) if G_u is None else np.asarray(G_u, dtype=float)
    A_p = kwf['Ad'] if Ap is None else np.asarray(Ap, dtype=float)
    B_p = kwf['Bd'] if Bp is None else np.asarray(Bp, dtype=float)
    if maps is None:                                       # (q, l, u are affine in the step data: one set of Jacobians serves every entry)
        maps = adjoint_ref.parameter_maps(entry_kwargs(kw, tape[0]), attrs)
    p = np.asarray(tape[0]['xref'], dtype=float).size
    lam = np.zeros((K + 1, nx)); lam[K] = G_x[K]
    mu = np.zeros(nu)
    res = dict(uref=np.zeros(nu), xref=np.zeros((K, p)), Ap=np.zeros((nx, nx)), Bp=np.zeros((nx, nu)),
               n_active=np.zeros(K, dtype=int), n_weak=np.zeros(K, dtype=int), status=np.zeros(K, dtype=int))
    model = {n: 0.0 for n in MODEL_NAMES}
    sets, last, n_factor, n_solved = [None] * K, None, 0, 0
    for k in range(K - 1, -1, -1):
        e = tape[k]
        g = G_u[k] + B_p.T @ lam[k + 1] + mu
        lam[k] = G_x[k] + A_p.T @ lam[k + 1]
        u_k = np.asarray(e['x'], dtype=float)[ou:ou + nu] if e['solved'] else kwf['uref']
        res['Ap'] += np.outer(lam[k + 1], e['x0'])
        res['Bp'] += np.outer(lam[k + 1], u_k)
        if not e['solved']:
            res['uref'] += g
            mu = np.zeros(nu)
            continue
        kwk = entry_kwargs(kw, e)
        if cache is None or k not in cache:
            (P, _, A, l, u), _ = adjoint_model_ref.build(kwk, attrs)
            if cache is not None:
                cache[k] = (P, A, l, u)
        else:
            P, A, l, u = cache[k]
        G = np.zeros(P.shape[0]); G[ou:ou + nu] = g
        r = adjoint_ref.adjoint(P, A, l, u, e['x'], e['z'], e['y'], D, E, c, G, maps, weak_tol=weak_tol)
        lam[k] += r['x0']
        mu = r['uminus1']
        res['uref'] += r['uref']
        res['xref'][k] = r['xref']
        gm, _ = adjoint_model_ref.closed_form_of(kwk, attrs, np.asarray(e['x'], dtype=float), np.asarray(e['y'], dtype=float), r['r_w'], r['r_y'])
        for n in MODEL_NAMES:
            model[n] = model[n] + gm[n]
        res['n_active'][k], res['n_weak'][k], res['status'][k] = r['n_active'], r['n_weak'], 1
        sets[k] = (r['low'].copy(), r['upp'].copy())
        n_solved += 1
        if last is None or not (np.array_equal(last[0], sets[k][0]) and np.array_equal(last[1], sets[k][1])):
            n_factor += 1
        last = sets[k]
    res.update(lam=lam, uminus1=mu, n_factor=n_factor, n_solved=n_solved, sets=sets)
    shapes = dict(Ad=(nx, nx), Bd=(nx, nu), Qx=(nx, nx), QxN=(nx, nx), Qu=(nu, nu), QDu=(nu, nu), eps_feas=())
    for n in MODEL_NAMES:
        res[n] = np.zeros(shapes[n]) + model[n]
    return res
