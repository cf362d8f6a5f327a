"""Restatement of the reverse sweep over an output-feedback rollout (include/mpcqp_rollout_est.h) for the tests: the recursion in numpy on
top of tests/adjoint_ref.py and tests/adjoint_model_ref.py, as tests/rollout_ref.py is for the state-feedback loop.  It shares nothing with
the HIP kernel (pympc_amd/csrc/mpcqp_rollout.h).

One instance at a time.  A tape is a list of entries of tests/rollout_ref.py -- x0 is the estimate xh_k the solve was made for -- with
x_plant [nx] = x_k and y_meas [ny] = y_k beside.  The loop is

    y_k = C x_k + v_k;  u_k = first input of entry k (uref where not solved);  x_{k+1} = Ap x_k + Bp u_k + w_k
    xh_{k+1} = Ad (xh_k + L (y_k - C xh_k)) + Bd u_k

and with the seeds G_x, G_xh [K+1, nx], G_u [K, nu], G_y [K, ny]:

    lam_K = G_x[K];  eta_K = G_xh[K];  mu = 0
    for k = K-1 .. 0:
        g = G_u[k] + Bp' lam_{k+1} + Bd' eta_{k+1} + mu;   s = Ad' eta_{k+1};   t = L' s;   r = G_y[k] + t
        lam_k = G_x[k] + Ap' lam_{k+1} + C' r;   eta_k = G_xh[k] + s - C' t (+ d_x0(g) if solved)
        solved: mu = d_um1(g), d_uref += d_uref(g), d_xref[k] = d_xref(g), model += model(g);   not solved: mu = 0, d_uref += g
        d_L += s (y_k - C xh_k)';  d_C += r x_k' - t xh_k';  d_v[k] = r
        d_Ap += lam_{k+1} x_k';  d_Bp += lam_{k+1} u_k';  d_Ae += eta_{k+1} (xh_k + L (y_k - C xh_k))';  d_Be += eta_{k+1} u_k'
    d_uminus1 = mu
"""
import numpy as np

import adjoint_ref
import adjoint_model_ref
import rollout_ref

MODEL_NAMES = adjoint_model_ref.NAMES


def sweep(kw, attrs, tape, D, E, c, C, L, G_x=None, G_xh=None, G_u=None, G_y=None, Ap=None, Bp=None, weak_tol=adjoint_ref.WEAK_TOL, maps=None, cache=None):
    """Everything mpcqp_rollout_adjoint_est returns for one instance: what tests/rollout_ref.py's sweep returns and eta [K+1, nx], C [ny, nx],
    L [nx, ny], v [K, ny], Ae [nx, nx], Be [nx, nu]."""
    attrs = attrs or {}
    K = len(tape)
    kwf = adjoint_model_ref.full_kwargs(kw)
    nx, nu = kwf['Bd'].shape
    ou = (kwf['Np'] + 1) * nx
    C, L = np.asarray(C, dtype=float), np.asarray(L, dtype=float)
    ny = C.shape[0]
    zero = lambda a, shape: np.zeros(shape) if a is None else np.asarray(a, dtype=float)
    G_x, G_xh, G_u, G_y = zero(G_x, (K + 1, nx)), zero(G_xh, (K + 1, nx)), zero(G_u, (K, nu)), zero(G_y, (K, ny))
    Ad, Bd = kwf['Ad'], kwf['Bd']
    A_p = Ad if Ap is None else np.asarray(Ap, dtype=float)
    B_p = Bd if Bp is None else np.asarray(Bp, dtype=float)
    if maps is None:
        maps = adjoint_ref.parameter_maps(rollout_ref.entry_kwargs(kw, tape[0]), attrs)
    p = np.asarray(tape[0]['xref'], dtype=float).size
    lam = np.zeros((K + 1, nx)); lam[K] = G_x[K]
    eta = np.zeros((K + 1, nx)); eta[K] = G_xh[K]
    mu = np.zeros(nu)
    res = dict(uref=np.zeros(nu), xref=np.zeros((K, p)), Ap=np.zeros((nx, nx)), Bp=np.zeros((nx, nu)), C=np.zeros((ny, nx)), L=np.zeros((nx, ny)),
               v=np.zeros((K, ny)), Ae=np.zeros((nx, nx)), Be=np.zeros((nx, nu)),
               n_active=np.zeros(K, dtype=int), n_weak=np.zeros(K, dtype=int), status=np.zeros(K, dtype=int))
    model = {n: 0.0 for n in MODEL_NAMES}
    sets, last, n_factor, n_solved = [None] * K, None, 0, 0
    for k in range(K - 1, -1, -1):
        e = tape[k]
        xh, xk, yk = (np.asarray(e[n], dtype=float) for n in ('x0', 'x_plant', 'y_meas'))
        u_k = np.asarray(e['x'], dtype=float)[ou:ou + nu] if e['solved'] else kwf['uref']
        g = G_u[k] + B_p.T @ lam[k + 1] + Bd.T @ eta[k + 1] + mu
        s = Ad.T @ eta[k + 1]
        t = L.T @ s
        r = G_y[k] + t
        inn = yk - C @ xh
        lam[k] = G_x[k] + A_p.T @ lam[k + 1] + C.T @ r
        eta[k] = G_xh[k] + s - C.T @ t
        res['L'] += np.outer(s, inn)
        res['C'] += np.outer(r, xk) - np.outer(t, xh)
        res['v'][k] = r
        res['Ap'] += np.outer(lam[k + 1], xk)
        res['Bp'] += np.outer(lam[k + 1], u_k)
        res['Ae'] += np.outer(eta[k + 1], xh + L @ inn)
        res['Be'] += np.outer(eta[k + 1], u_k)
        if not e['solved']:
            res['uref'] += g
            mu = np.zeros(nu)
            continue
        kwk = rollout_ref.entry_kwargs(kw, e)
        if cache is None or k not in cache:
            (P, _, A, l, u), _ = adjoint_model_ref.build(kwk, attrs)
            if cache is not None:
                cache[k] = (P, A, l, u)
        else:
            P, A, l, u = cache[k]
        G = np.zeros(P.shape[0]); G[ou:ou + nu] = g
        a = adjoint_ref.adjoint(P, A, l, u, e['x'], e['z'], e['y'], D, E, c, G, maps, weak_tol=weak_tol)
        eta[k] += a['x0']
        mu = a['uminus1']
        res['uref'] += a['uref']
        res['xref'][k] = a['xref']
        gm, _ = adjoint_model_ref.closed_form_of(kwk, attrs, np.asarray(e['x'], dtype=float), np.asarray(e['y'], dtype=float), a['r_w'], a['r_y'])
        for n in MODEL_NAMES:
            model[n] = model[n] + gm[n]
        res['n_active'][k], res['n_weak'][k], res['status'][k] = a['n_active'], a['n_weak'], 1
        sets[k] = (a['low'].copy(), a['upp'].copy())
        n_solved += 1
        if last is None or not (np.array_equal(last[0], sets[k][0]) and np.array_equal(last[1], sets[k][1])):
            n_factor += 1
        last = sets[k]
    res.update(lam=lam, eta=eta, uminus1=mu, n_factor=n_factor, n_solved=n_solved, sets=sets)
    shapes = dict(Ad=(nx, nx), Bd=(nx, nu), Qx=(nx, nx), QxN=(nx, nx), Qu=(nu, nu), QDu=(nu, nu), eps_feas=())
    for n in MODEL_NAMES:
        res[n] = np.zeros(shapes[n]) + model[n]
    return res
