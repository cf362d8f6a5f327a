"""Restatement of the reverse sweep over a closed-loop rollout with an affine term in the prediction model, x+ = Ad x + Bd u + d
(include_ext5/mpcqp_rollout_affine.h) for the tests: the recursion of tests/rollout_ref.py / tests/rollout_tv_ref.py with the term of slot
tau(k) on the dynamics rows of entry k, in numpy on top of tests/adjoint_ref.py and tests/adjoint_model_ref.py.  It shares nothing with the
HIP kernel (pympc_amd/csrc/mpcqp_rollout.h).

One instance at a time.  A tape is a list of entries as in tests/rollout_ref.py.  ``d_slots`` [nslots, rows, nx] (rows: 1 or Np): slot 0 the
term the rollout began under (zeros: none), slot e + 1 schedule entry e; ``d_hold``: steps per entry, 0 for one constant term (one slot).
``slots``: the model slots of tests/rollout_tv_ref.py under a model schedule of ``hold`` steps per entry, or ONE dict(Ad, Bd, D, E, c) in a
list without one (hold = 0).  With tau(k) = 0 for k = 0 or d_hold = 0, 1 + (k - 1) // d_hold beyond:

    the recursion of tests/rollout_tv_ref.py, where the QP of entry k has  l = u = 0.0 - d_slots[tau(k)][j]  on the rows of stage j + 1, and
    solved:   d_slots_grad[tau(k)] += -(d_l) of those rows  (rows = 1: summed over the stages in ascending order)
"""
import numpy as np

import adjoint_ref
import adjoint_model_ref
import rollout_ref
import rollout_tv_ref

WEIGHT_NAMES = rollout_tv_ref.WEIGHT_NAMES


def tau(k, d_hold):
    """The term slot the solve of tape entry k was made under."""
    return 0 if (k == 0 or d_hold == 0) else 1 + (k - 1) // d_hold


def with_term(l, u, d, nx, Np):
    """Copies of (l, u) with 0.0 - d_j on the rows of stage j + 1; d [rows, nx], rows 1 or Np."""
    l, u = np.array(l, dtype=float), np.array(u, dtype=float)
    rows = 0.0 - np.broadcast_to(np.asarray(d, dtype=float).reshape(-1, nx), (Np, nx)).ravel()
    l[nx:(Np + 1) * nx] = rows
    u[nx:(Np + 1) * nx] = rows
    return l, u


def sweep(kw, attrs, tape, d_slots, d_hold, slots, hold=0, G_x=None, G_u=None, Ap=None, Bp=None, weak_tol=adjoint_ref.WEAK_TOL, bmaps=None, maps=None):
    """Everything mpcqp_rollout_adjoint_affine returns for one instance: what tests/rollout_tv_ref.sweep returns (without a model schedule
    Ad_slots, Bd_slots have one slot and Ap_entries, Bp_entries one entry: the sums of tests/rollout_ref.py) and d_slots [nslots, rows, nx]."""
    attrs = attrs or {}
    K = len(tape)
    sched = hold > 0
    nseg = (K + hold - 1) // hold if sched else 1
    assert len(slots) == (nseg + 1 if sched else 1)
    d_slots = np.asarray(d_slots, dtype=float)
    nslots, rows = d_slots.shape[0], d_slots.shape[1]
    assert nslots == ((K + d_hold - 1) // d_hold + 1 if d_hold else 1)
    kwf = adjoint_model_ref.full_kwargs(kw)
    nx, nu = kwf['Bd'].shape
    Np = kwf['Np']
    assert rows in (1, Np)
    ou = (Np + 1) * nx
    G_x = np.zeros((K + 1, nx)) if G_x is None else np.asarray(G_x, dtype=float)
    G_u = np.zeros((K, nu)) if G_u is None else np.asarray(G_u, dtype=float)
    p = np.asarray(tape[0]['xref'], dtype=float).size
    lam = np.zeros((K + 1, nx)); lam[K] = G_x[K]
    mu = np.zeros(nu)
    nms = nseg + 1 if sched else 1
    res = dict(uref=np.zeros(nu), xref=np.zeros((K, p)), Ad_slots=np.zeros((nms, nx, nx)), Bd_slots=np.zeros((nms, nx, nu)),
               Ap_entries=np.zeros((nseg, nx, nx)), Bp_entries=np.zeros((nseg, nx, nu)), d_slots=np.zeros((nslots, rows, nx)),
               n_active=np.zeros(K, dtype=int), n_weak=np.zeros(K, dtype=int), status=np.zeros(K, dtype=int))
    weights = {n: 0.0 for n in WEIGHT_NAMES}
    bounds = None if bmaps is None else {n: np.zeros(J[0].shape[1]) for n, J in bmaps.items()}
    maps = {} if maps is None else maps                    # (model slot -> the Jacobians of q, l, u in the step data; the term does not enter them: a caller may keep them)
    sets, last, n_factor = [None] * K, None, 0
    for k in range(K - 1, -1, -1):
        e = tape[k]
        s = rollout_tv_ref.sigma(k, hold) if sched else 0
        seg = k // hold if sched else 0
        inforce = slots[1 + seg] if sched else slots[0]
        t = tau(k, d_hold)
        A_p = np.asarray(inforce['Ad'] if Ap is None else Ap, dtype=float)
        B_p = np.asarray(inforce['Bd'] if Bp is None else Bp, dtype=float)
        g = G_u[k] + B_p.T @ lam[k + 1] + mu
        lam[k] = G_x[k] + A_p.T @ lam[k + 1]
        u_k = np.asarray(e['x'], dtype=float)[ou:ou + nu] if e['solved'] else kwf['uref']
        res['Ap_entries'][seg] += np.outer(lam[k + 1], e['x0'])
        res['Bp_entries'][seg] += np.outer(lam[k + 1], u_k)
        if not e['solved']:
            res['uref'] += g
            mu = np.zeros(nu)
            continue
        kwk = rollout_ref.entry_kwargs(rollout_tv_ref.with_slot(kw, slots[s]), e)
        if s not in maps:
            maps[s] = adjoint_ref.parameter_maps(kwk, attrs)
        (P, _, A, l, u), _ = adjoint_model_ref.build(kwk, attrs)
        l, u = with_term(l, u, d_slots[t], nx, Np)
        G = np.zeros(P.shape[0]); G[ou:ou + nu] = g
        r = adjoint_ref.adjoint(P, A, l, u, e['x'], e['z'], e['y'], slots[s]['D'], slots[s]['E'], slots[s]['c'], G, maps[s], weak_tol=weak_tol)
        lam[k] += r['x0']
        mu = r['uminus1']
        res['uref'] += r['uref']
        res['xref'][k] = r['xref']
        dd = -(np.asarray(r['d_l'], dtype=float) + np.asarray(r['d_u'], dtype=float))[nx:(Np + 1) * nx].reshape(Np, nx)      # (l = u = 0.0 - d)
        if rows == 1:
            acc = np.zeros(nx)
            for j in range(Np):
                acc = acc + dd[j]
            dd = acc[None]
        res['d_slots'][t] += dd
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
