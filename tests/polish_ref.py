"""Dense restatement of OSQP's solution polishing (OSQP 0.6, polish.c) for the tests: numpy / scipy only, sharing nothing with
the HIP kernel (pympc_amd/csrc/mpcqp_polish.h).

Everything happens in a given scaling (D, E, c) of the problem, as in OSQP:
    P~ = c D P D,  q~ = c D q,  A~ = E A D,  l~ = E l,  u~ = E u,  x~ = x / D,  z~ = E z,  y~ = c y / E.
1. active set from the iterate (x, z, y):  lower-active if z~ - l~ < -y~, else upper-active if u~ - z~ < y~;
2. the regularized reduced KKT system [[P~ + delta I, A~r'], [A~r, -delta I]] [x~; y~r] = [-q~; b~r] (b = l or u of each active
   row) solved directly, then `refine_iter` steps of iterative refinement against the UNREGULARIZED matrix [[P~, A~r'], [A~r, 0]];
3. y = multiplier on the active rows, 0 elsewhere; z = clip(A x, l, u);
4. accepted iff (pri_pol < pri and dua_pol < dua) or (pri_pol < pri and dua < 1e-10) or (dua_pol < dua and pri < 1e-10), with the
   unscaled residuals |A x - z|_inf and |P x + q + A'y|_inf.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

QP_INFTY = 1e30

# fixtures on which polishing the oracle's eps-1e-3 iterate reaches x* to 1e-8 (measured by tests/test_polish_reference.py)
EXACT = ['cart_pole_nc1', 'point_mass', 'point_mass_hard', 'point_mass_nc', 'quadcopter_nc', 'quadcopter_nodu', 'random_12_4_30',
         'random_12_4_30_b', 'random_12_4_30_hard', 'random_20_8_12_hard', 'random_5_3_8_nc', 'random_5_3_8_nc_hard', 'small_mimo']
# ... and on which it is accepted (EXACT and these)
ACCEPTED = EXACT + ['accel_brake', 'accel_brake_hard', 'cart_pole', 'cart_pole_kalman']
# the same with the oracle's default Ruiz scaling and its own (D, E, c) -- what the device does: the same fixtures are accepted; the iterate the
# scaled iteration stops at gets the active set right (x* to 1e-8) on these
EXACT_SCALED = ['accel_brake', 'accel_brake_hard', 'point_mass_nc', 'quadcopter_nc', 'quadcopter_nodu', 'random_12_4_30', 'random_12_4_30_b',
                'random_12_4_30_hard', 'random_20_8_12_hard', 'random_5_3_8_nc', 'random_5_3_8_nc_hard', 'small_mimo']


def active_set(A, l, u, x, z, y, D, E, c):
    """OSQP's rule in the scaling (D, E, c): (lower-active mask, upper-active mask)."""
    zs, ls, us, ys = E * z, E * np.clip(l, -QP_INFTY, QP_INFTY), E * np.clip(u, -QP_INFTY, QP_INFTY), c * y / E
    low = zs - ls < -ys
    upp = ~low & (us - zs < ys)
    return low, upp


def residuals(P, q, A, l, u, x, z, y):
    """(pri_res, dua_res, obj_val) in unscaled units, as the termination test reports them."""
    pri = np.abs(A @ x - z).max() if A.shape[0] else 0.0
    dua = np.abs(P @ x + q + A.T @ y).max()
    return pri, dua, 0.5 * x @ (P @ x) + q @ x


def polish(P, q, A, l, u, x, z, y, D, E, c, pri, dua, delta=1e-6, refine_iter=3):
    """Polish the iterate (x, z, y) (unscaled) of a solve that ended with residuals (pri, dua).  Returns a dict with the
    polished x, y, z, the active masks, the residuals of the polished point and `status_polish` (1 accepted, -1 rejected)."""
    P, A = sp.csr_matrix(P), sp.csr_matrix(A)
    n = P.shape[0]
    lc, uc = np.clip(l, -QP_INFTY, QP_INFTY), np.clip(u, -QP_INFTY, QP_INFTY)
    low, upp = active_set(A, l, u, x, z, y, D, E, c)
    act = np.flatnonzero(low | upp)
    b = np.where(low, lc, uc)[act]
    Dm, Em = sp.diags(D), sp.diags(E)
    Ps = (c * (Dm @ P @ Dm)).tocsc()
    qs = c * D * q
    Ar = (Em @ A @ Dm).tocsr()[act]
    bs = E[act] * b
    k = len(act)
    K0 = sp.bmat([[Ps, Ar.T], [Ar, None]], format='csc') if k else Ps.tocsc()
    Kd = (K0 + sp.diags(np.r_[np.full(n, delta), np.full(k, -delta)])).tocsc()
    rhs = np.r_[-qs, bs]
    lu = spla.splu(Kd)
    sol = lu.solve(rhs)
    for _ in range(refine_iter):
        sol = sol + lu.solve(rhs - K0 @ sol)
    xp = D * sol[:n]
    yp = np.zeros(A.shape[0])
    yp[act] = E[act] * sol[n:] / c
    zp = np.clip(A @ xp, lc, uc)
    pp, dp, op = residuals(P, q, A, l, u, xp, zp, yp)
    ok = (pp < pri and dp < dua) or (pp < pri and dua < 1e-10) or (dp < dua and pri < 1e-10)
    return dict(x=xp, y=yp, z=zp, low=low, upp=upp, pri_res=pp, dua_res=dp, obj_val=op, status_polish=1 if ok else -1)


def golden_qp(g):
    """(P full symmetric, q, A, l, u) of a tests/golden/qp_*.npz fixture."""
    from util import golden_csc
    U = sp.triu(golden_csc(g, 'P'), format='csc')
    return (U + sp.triu(U, 1).T).tocsc(), np.asarray(g['q'], dtype=float), golden_csc(g, 'A').tocsc(), \
        np.asarray(g['l'], dtype=float), np.asarray(g['u'], dtype=float)


# ---- the device against this restatement (tests/test_gpu_polish.py, tests/test_gpu_row_types.py) -----------------------------------
def device_spec(bp, b=0):
    """polish_ref on instance b of BatchProblem bp, from the iterate and scaling the device holds now."""
    P, q, A, l, u = (v[b] for v in bp.export_qp())
    x, z, y = (v[b] for v in bp.iterate_state())
    D, E, c, _ = bp.scaling()
    info = bp.infos()[b]
    return polish(P, q, A, l, u, x, z, y, D[b], E[b], c[b], info.pri_res, info.dua_res)


def check_against_spec(bp, idx=None):
    """Polish the last solve of bp (polish off until now) and compare every instance in idx with polish_ref."""
    import pytest
    from util import rel1
    idx = range(bp.batch) if idx is None else idx
    refs = {b: device_spec(bp, b) for b in idx}
    bp.polish()
    st = bp.polish_status()
    x, y, info = bp.solution()
    for b, ref in refs.items():
        assert st[b] == ref['status_polish'], (b, st[b], ref['status_polish'])
        if st[b] == 1:
            assert rel1(x[b], ref['x']) <= 1e-9, (b, rel1(x[b], ref['x']))
            # (the multipliers come out of (omega / c) (A x - b) with omega / c ~ E^2 / (c delta): the rounding of A x - b, 1e6 times)
            assert rel1(y[b], ref['y']) <= 1e-8, (b, rel1(y[b], ref['y']))
            assert np.all(y[b][~(ref['low'] | ref['upp'])] == 0.0), (b, 'multipliers off the active set')
            assert info[b].pri_res == pytest.approx(ref['pri_res'], abs=1e-9 * max(1.0, np.abs(ref['x']).max())), (b, info[b].pri_res, ref['pri_res'])
    return st
