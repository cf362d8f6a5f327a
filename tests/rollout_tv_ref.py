"""Restatement of the reverse sweep over a closed-loop rollout under a model schedule (include_ext/mpcqp_rollout_tv.h) for the tests: the
recursion of tests/rollout_ref.py with a model and a scaling per tape entry, in numpy on top of tests/adjoint_ref.py and
tests/adjoint_model_ref.py.  It shares nothing with the HIP kernel (pympc_amd/csrc/mpcqp_rollout.h).

One instance at a time.  A tape is a list of entries as in tests/rollout_ref.py; ``slots`` is a list of nseg + 1 dicts
dict(Ad, Bd, D, E, c): slot 0 the model the rollout began under, slot e + 1 schedule entry e, each with the scaling the solver
equilibrated it to.  With sigma(k) = 0 for k = 0, 1 + (k - 1) // hold beyond (the slot the solve of entry k was made under) and
pi(k) = 1 + k // hold (the slot in force at step k, the plant's where none is given):

    lam_K = G_x[K];  mu = 0
    for k = K-1 .. 0:
        (Ap, Bp) = the given plant, or (Ad, Bd) of slot pi(k)
        g      = G_u[k] + Bp' lam_{k+1} + mu
        solved:      the adjoint of entry k under slot sigma(k) with seed g:  lam_k = G_x[k] + Ap' lam_{k+1} + d_x0;  mu = d_um1;
                     d_uref += ..;  d_xref[k] = ..;  weights += ..;  Ad_slots[sigma(k)] += d_Ad;  Bd_slots[sigma(k)] += d_Bd
        not solved:  lam_k = G_x[k] + Ap' lam_{k+1};  mu = 0;  d_uref += g
        Ap_entries[k // hold] += lam_{k+1} x_k';   Bp_entries[k // hold] += lam_{k+1} u_k'
    d_uminus1 = mu
"""
import numpy as np

import adjoint_ref
import adjoint_model_ref
import rollout_ref

WEIGHT_NAMES = ('Qx', 'QxN', 'Qu', 'QDu', 'eps_feas')


def sigma(k, hold):
    """The slot the solve of tape entry k was made under."""
    return 0 if k == 0 else 1 + (k - 1) // hold


def with_slot(kw, slot):
    """The controller's kwargs (every field given) with the slot's Ad, Bd."""
    k2 = adjoint_model_ref.full_kwargs(kw)
    k2['Ad'], k2['Bd'] = np.array(slot['Ad'], dtype=float), np.array(slot['Bd'], dtype=float)
    return k2


def sweep(kw, attrs, tape, slots, hold, G_x=None, G_u=None, Ap=None, Bp=None, weak_tol=adjoint_ref.WEAK_TOL, bmaps=None):
    """Everything mpcqp_rollout_adjoint_tv returns for one instance: dict lam [K+1, nx], uminus1, uref [nu], xref [K, p], Ad_slots
    [nseg+1, nx, nx], Bd_slots [nseg+1, nx, nu], Ap_entries [nseg, nx, nx], Bp_entries [nseg, nx, nu], the five weight gradients, n_active,
    n_weak, status [K], n_factor (1 + the changes of active set or slot along the solved entries, in sweep order) and sets [K]; with
    ``bmaps`` (tests/bounds_ref.bound_maps: the bounds do not change along a schedule) the six bound gradients too."""
    attrs = attrs or {}
    K = len(tape)
    nseg = (K + hold - 1) // hold
    assert len(slots) == nseg + 1
    kwf = adjoint_model_ref.full_kwargs(kw)
    nx, nu = kwf['Bd'].shape
    ou = (kwf['Np'] + 1) * nx
    G_x = np.zeros((K + 1, nx)) if G_x is None else np.asarray(G_x, dtype=float)
    G_u = np.zeros((K, nu)) if G_u is None else np.asarray(G_u, dtype=float)
    p = np.asarray(tape[0]['xref'], dtype=float).size
    lam = np.zeros((K + 1, nx)); lam[K] = G_x[K]
    mu = np.zeros(nu)
    res = dict(uref=np.zeros(nu), xref=np.zeros((K, p)), Ad_slots=np.zeros((nseg + 1, nx, nx)), Bd_slots=np.zeros((nseg + 1, nx, nu)),
               Ap_entries=np.zeros((nseg, nx, nx)), Bp_entries=np.zeros((nseg, nx, nu)),
               n_active=np.zeros(K, dtype=int), n_weak=np.zeros(K, dtype=int), status=np.zeros(K, dtype=int))
    weights = {n: 0.0 for n in WEIGHT_NAMES}
    bounds = None if bmaps is None else {n: np.zeros(J[0].shape[1]) for n, J in bmaps.items()}
    maps = {}                                              # (q, l, u are affine in the step data under ONE model: a set of Jacobians per slot)
    sets, last, n_factor = [None] * K, None, 0
    for k in range(K - 1, -1, -1):
        e = tape[k]
        s, inforce = sigma(k, hold), slots[1 + k // hold]
        A_p = np.asarray(inforce['Ad'] if Ap is None else Ap, dtype=float)
        B_p = np.asarray(inforce['Bd'] if Bp is None else Bp, dtype=float)
        g = G_u[k] + B_p.T @ lam[k + 1] + mu
        lam[k] = G_x[k] + A_p.T @ lam[k + 1]
        u_k = np.asarray(e['x'], dtype=float)[ou:ou + nu] if e['solved'] else kwf['uref']
        res['Ap_entries'][k // hold] += np.outer(lam[k + 1], e['x0'])
        res['Bp_entries'][k // hold] += np.outer(lam[k + 1], u_k)
        if not e['solved']:
            res['uref'] += g
            mu = np.zeros(nu)
            continue
        kws = with_slot(kw, slots[s])
        kwk = rollout_ref.entry_kwargs(kws, e)
        if s not in maps:
            maps[s] = adjoint_ref.parameter_maps(kwk, attrs)
        (P, _, A, l, u), _ = adjoint_model_ref.build(kwk, attrs)
        G = np.zeros(P.shape[0]); G[ou:ou + nu] = g
        r = adjoint_ref.adjoint(P, A, l, u, e['x'], e['z'], e['y'], slots[s]['D'], slots[s]['E'], slots[s]['c'], G, maps[s], weak_tol=weak_tol)
        lam[k] += r['x0']
        mu = r['uminus1']
        res['uref'] += r['uref']
        res['xref'][k] = r['xref']
        gm, _ = adjoint_model_ref.closed_form_of(kwk, attrs, np.asarray(e['x'], dtype=float), np.asarray(e['y'], dtype=float), r['r_w'], r['r_y'])
        res['Ad_slots'][s] += gm['Ad']
        res['Bd_slots'][s] += gm['Bd']
        for n in WEIGHT_NAMES:
            weights[n] = weights[n] + gm[n]
        if bounds is not None:
            for n, (Jl, Ju) in bmaps.items():
                bounds[n] = bounds[n] + Jl.T @ np.asarray(r['d_l'], dtype=float) + Ju.T @ np.asarray(r['d_u'], dtype=float)
        res['n_active'][k], res['n_weak'][k], res['status'][k] = r['n_active'], r['n_weak'], 1
        sets[k] = (r['low'].copy(), r['upp'].copy(), s)
        if last is None or last[2] != s or not (np.array_equal(last[0], sets[k][0]) and np.array_equal(last[1], sets[k][1])):
            n_factor += 1
        last = sets[k]
    res.update(lam=lam, uminus1=mu, n_factor=n_factor, sets=sets)
    res.update(bounds or {})
    shapes = dict(Qx=(nx, nx), QxN=(nx, nx), Qu=(nu, nu), QDu=(nu, nu), eps_feas=())
    for n in WEIGHT_NAMES:
        res[n] = np.zeros(shapes[n]) + weights[n]
    return res
