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
