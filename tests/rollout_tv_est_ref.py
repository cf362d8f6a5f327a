"""Restatement of the reverse sweep over an output-feedback rollout under a model schedule (include_ext2/mpcqp_rollout_tv_est.h) for the
tests: the recursion of tests/rollout_est_ref.py with the slots of tests/rollout_tv_ref.py and a gain per schedule entry, in numpy on top of
tests/adjoint_ref.py and tests/adjoint_model_ref.py.  It shares nothing with the HIP kernel (pympc_amd/csrc/mpcqp_rollout.h).

One instance at a time.  A tape is a list of entries as tests/rollout_est_ref.py takes them (x0 = the estimate xh_k, x_plant, y_meas beside);
``slots`` the nseg + 1 dicts dict(Ad, Bd, D, E, c) of tests/rollout_tv_ref.py; ``gains`` [nseg, nx, ny] the gain of every entry.  With
e(k) = k // hold, pi(k) = 1 + e(k) and sigma(k) = rollout_tv_ref.sigma(k, hold):

    lam_K = G_x[K];  eta_K = G_xh[K];  mu = 0
    for k = K-1 .. 0:
        (Ad, Bd) = slot pi(k);  L = gains[e(k)];  (Ap, Bp) = the given plant, or (Ad, Bd)
        g = G_u[k] + Bp' lam_{k+1} + Bd' eta_{k+1} + mu;   s = Ad' eta_{k+1};   t = L' s;   r = G_y[k] + t
        lam_k = G_x[k] + Ap' lam_{k+1} + C' r;   eta_k = G_xh[k] + s - C' t (+ d_x0(g) if solved)
        solved: the adjoint of entry k under slot sigma(k): mu = d_um1, d_uref += .., d_xref[k] = .., weights += .., Ad_slots[sigma(k)] += d_Ad,
                Bd_slots[sigma(k)] += d_Bd;   not solved: mu = 0, d_uref += g
        L_entries[e(k)] += s (y_k - C xh_k)';  d_C += r x_k' - t xh_k';  d_v[k] = r
        Ap_entries[e(k)] += lam_{k+1} x_k';  Bp_entries[e(k)] += lam_{k+1} u_k'
        Ae_entries[e(k)] += eta_{k+1} (xh_k + L (y_k - C xh_k))';  Be_entries[e(k)] += eta_{k+1} u_k'
    d_uminus1 = mu
"""
import numpy as np

import adjoint_ref
import adjoint_model_ref
import rollout_ref
import rollout_tv_ref

WEIGHT_NAMES = rollout_tv_ref.WEIGHT_NAMES


def sweep(kw, attrs, tape, slots, hold, C, gains, G_x=None, G_xh=None, G_u=None, G_y=None, Ap=None, Bp=None, weak_tol=adjoint_ref.WEAK_TOL, bmaps=None):
    """Everything mpcqp_rollout_adjoint_tv_est returns for one instance: what tests/rollout_tv_ref.py's sweep returns, eta [K+1, nx], C [ny, nx],
    v [K, ny] and Ae_entries [nseg, nx, nx], Be_entries [nseg, nx, nu], L_entries [nseg, nx, ny]."""
    attrs = attrs or {}
    K = len(tape)
    nseg = (K + hold - 1) // hold
    assert len(slots) == nseg + 1 and len(gains) >= nseg
    kwf = adjoint_model_ref.full_kwargs(kw)
    nx, nu = kwf['Bd'].shape
    ou = (kwf['Np'] + 1) * nx
    C = np.asarray(C, dtype=float)
    ny = C.shape[0]
    zero = lambda a, shape: np.zeros(shape) if a is None else np.asarray(a, dtype=float)
    G_x, G_xh, G_u, G_y = zero(G_x, (K + 1, nx)), zero(G_xh, (K + 1, nx)), zero(G_u, (K, nu)), zero(G_y, (K, ny))
    p = np.asarray(tape[0]['xref'], dtype=float).size
    lam = np.zeros((K + 1, nx)); lam[K] = G_x[K]
    eta = np.zeros((K + 1, nx)); eta[K] = G_xh[K]
    mu = np.zeros(nu)
    res = dict(uref=np.zeros(nu), xref=np.zeros((K, p)), Ad_slots=np.zeros((nseg + 1, nx, nx)), Bd_slots=np.zeros((nseg + 1, nx, nu)),
               Ap_entries=np.zeros((nseg, nx, nx)), Bp_entries=np.zeros((nseg, nx, nu)), Ae_entries=np.zeros((nseg, nx, nx)),
               Be_entries=np.zeros((nseg, nx, nu)), L_entries=np.zeros((nseg, nx, ny)), C=np.zeros((ny, nx)), v=np.zeros((K, ny)),
               n_active=np.zeros(K, dtype=int), n_weak=np.zeros(K, dtype=int), status=np.zeros(K, dtype=int))
    weights = {n: 0.0 for n in WEIGHT_NAMES}
    bounds = None if bmaps is None else {n: np.zeros(J[0].shape[1]) for n, J in bmaps.items()}
    maps = {}
    sets, last, n_factor = [None] * K, None, 0
    for k in range(K - 1, -1, -1):
        e = tape[k]
        en = k // hold
        sg, inforce = rollout_tv_ref.sigma(k, hold), slots[1 + en]
        Ad, Bd, L = np.asarray(inforce['Ad'], dtype=float), np.asarray(inforce['Bd'], dtype=float), np.asarray(gains[en], dtype=float)
        A_p = Ad if Ap is None else np.asarray(Ap, dtype=float)
        B_p = Bd if Bp is None else np.asarray(Bp, dtype=float)
        xh, xk, yk = (np.asarray(e[n], dtype=float) for n in ('x0', 'x_plant', 'y_meas'))
        u_k = np.asarray(e['x'], dtype=float)[ou:ou + nu] if e['solved'] else kwf['uref']
        g = G_u[k] + B_p.T @ lam[k + 1] + Bd.T @ eta[k + 1] + mu
        s = Ad.T @ eta[k + 1]
        t = L.T @ s
        r = G_y[k] + t
        inn = yk - C @ xh
        lam[k] = G_x[k] + A_p.T @ lam[k + 1] + C.T @ r
        eta[k] = G_xh[k] + s - C.T @ t
        res['L_entries'][en] += np.outer(s, inn)
        res['C'] += np.outer(r, xk) - np.outer(t, xh)
        res['v'][k] = r
        res['Ap_entries'][en] += np.outer(lam[k + 1], xk)
        res['Bp_entries'][en] += np.outer(lam[k + 1], u_k)
        res['Ae_entries'][en] += np.outer(eta[k + 1], xh + L @ inn)
        res['Be_entries'][en] += np.outer(eta[k + 1], u_k)
        if not e['solved']:
            res['uref'] += g
            mu = np.zeros(nu)
            continue
        kws = rollout_tv_ref.with_slot(kw, slots[sg])
        kwk = rollout_ref.entry_kwargs(kws, e)
        if sg not in maps:
            maps[sg] = adjoint_ref.parameter_maps(kwk, attrs)
        (P, _, A, l, u), _ = adjoint_model_ref.build(kwk, attrs)
        G = np.zeros(P.shape[0]); G[ou:ou + nu] = g
        a = adjoint_ref.adjoint(P, A, l, u, e['x'], e['z'], e['y'], slots[sg]['D'], slots[sg]['E'], slots[sg]['c'], G, maps[sg], weak_tol=weak_tol)
        eta[k] += a['x0']
        mu = a['uminus1']
        res['uref'] += a['uref']
        res['xref'][k] = a['xref']
        gm, _ = adjoint_model_ref.closed_form_of(kwk, attrs, np.asarray(e['x'], dtype=float), np.asarray(e['y'], dtype=float), a['r_w'], a['r_y'])
        res['Ad_slots'][sg] += gm['Ad']
        res['Bd_slots'][sg] += gm['Bd']
        for n in WEIGHT_NAMES:
            weights[n] = weights[n] + gm[n]
        if bounds is not None:
            for n, (Jl, Ju) in bmaps.items():
                bounds[n] = bounds[n] + Jl.T @ np.asarray(a['d_l'], dtype=float) + Ju.T @ np.asarray(a['d_u'], dtype=float)
        res['n_active'][k], res['n_weak'][k], res['status'][k] = a['n_active'], a['n_weak'], 1
        sets[k] = (a['low'].copy(), a['upp'].copy(), sg)
        if last is None or last[2] != sg or not (np.array_equal(last[0], sets[k][0]) and np.array_equal(last[1], sets[k][1])):
            n_factor += 1
        last = sets[k]
    res.update(lam=lam, eta=eta, uminus1=mu, n_factor=n_factor, sets=sets)
    res.update(bounds or {})
    shapes = dict(Qx=(nx, nx), QxN=(nx, nx), Qu=(nu, nu), QDu=(nu, nu), eps_feas=())
    for n in WEIGHT_NAMES:
        res[n] = np.zeros(shapes[n]) + weights[n]
    return res
