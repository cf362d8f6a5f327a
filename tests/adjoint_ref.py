"""Restatement of the adjoint derivatives of the MPC solution (include/mpcqp_adjoint.h) for the tests: numpy / scipy sparse LU only,
sharing nothing with the HIP kernel (pympc_amd/csrc/mpcqp_adjoint.h).

The QP is  min 1/2 w'P w + q'w,  l <= A w <= u.  With the active rows a (every equality row l == u, plus the rows OSQP's polishing rule
marks active on the iterate, tests/polish_ref.py) and b the bound each sits on, w* locally solves  [P, A_a'; A_a, 0] [w; y_a] = [-q; b].
For a seed g = dL/dw:   [P, A_a'; A_a, 0] [r_w; r_y] = [g; 0],   dL/dq = -r_w,   dL/db_i = r_y[i] on active rows, 0 elsewhere.
The system is solved UNREGULARIZED by a sparse LU (in the scaling (D, E, c) it is given, for conditioning) with two steps of iterative
refinement -- not by the regularized factor and multiplier sweeps of the kernel.

The chain into the controller's parameters is not written down here at all: q, l, u are affine in (x0, u_{-1}, xref, uref), so their
Jacobians are read off the host builder itself (pympc_amd.qp_build through MPCController._compute_QP_matrices_, i.e. pyMPC/mpc.py:386-452)
by moving one parameter entry at a time by one unit.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from polish_ref import active_set as polish_active_set

QP_INFTY = 1e30
WEAK_TOL = 1e-6


def active_rows(A, l, u, x, z, y, D, E, c):
    """(lower-active or equality mask, upper-active mask): polishing's rule on the iterate, and every equality row."""
    low, upp = polish_active_set(A, l, u, x, z, y, D, E, c)
    eq = np.clip(l, -QP_INFTY, QP_INFTY) == np.clip(u, -QP_INFTY, QP_INFTY)
    low = low | eq
    return low, upp & ~low


def count_weak(l, u, z, y, weak_tol=WEAK_TOL):
    """Rows with l != u on a bound with a zero multiplier (unscaled units): min(z - l, u - z) <= tol max(1, |z_i|) and
    |y_i| <= tol max(1, |y|_inf)."""
    lc, uc = np.clip(l, -QP_INFTY, QP_INFTY), np.clip(u, -QP_INFTY, QP_INFTY)
    on = np.minimum(z - lc, uc - z) <= weak_tol * np.maximum(1.0, np.abs(z))
    zero = np.abs(y) <= weak_tol * max(1.0, np.abs(y).max() if y.size else 0.0)
    return int(np.count_nonzero((lc != uc) & on & zero))


def exact_active_rows(A, l, u, x, y, tol=1e-7):
    """The active set of a SOLUTION (x, y) known to high accuracy: equality rows, and rows on a bound with a non-zero multiplier."""
    lc, uc = np.clip(l, -QP_INFTY, QP_INFTY), np.clip(u, -QP_INFTY, QP_INFTY)
    ys = tol * max(1.0, np.abs(y).max())
    eq = lc == uc
    low = eq | (y < -ys)
    upp = ~low & (y > ys)
    return low, upp


def solve_adjoint(P, A, low, upp, G, D=None, E=None, c=1.0, refine=2):
    """(R_w [n, k], R_y [m, k]) for the seeds G [n, k] (or one seed [n]): the active-set KKT system, sparse LU, unregularized."""
    P, A = sp.csc_matrix(P), sp.csr_matrix(A)
    n, m = P.shape[0], A.shape[0]
    one = np.ndim(G) == 1
    G = np.asarray(G, dtype=float).reshape(n, -1)
    D = np.ones(n) if D is None else np.asarray(D, dtype=float)
    E = np.ones(m) if E is None else np.asarray(E, dtype=float)
    act = np.flatnonzero(low | upp)
    Dm = sp.diags(D)
    Ps = c * (Dm @ P @ Dm)
    Ar = (sp.diags(E[act]) @ A[act] @ Dm) if len(act) else sp.csr_matrix((0, n))
    K = sp.bmat([[Ps, Ar.T], [Ar, None]], format='csc') if len(act) else Ps.tocsc()
    rhs = np.vstack([c * D[:, None] * G, np.zeros((len(act), G.shape[1]))])
    try:
        lu = spla.splu(K)
        sol = lu.solve(rhs)
        for _ in range(refine):
            sol = sol + lu.solve(rhs - K @ sol)
        if not np.isfinite(sol).all():
            raise RuntimeError('singular')
    except RuntimeError:
        # linearly dependent active rows (pyMPC's Delta-u rows couple neighbouring scalars: u_0, u_1 - u_0, u_2 - u_1 and u_2 can all sit on
        # bounds): the system is consistent but singular, r_w is still unique, r_y is not -- take the minimum-norm solution
        sol = np.linalg.lstsq(K.toarray(), rhs, rcond=1e-13)[0]
    Rw = D[:, None] * sol[:n]
    Ry = np.zeros((m, G.shape[1]))
    Ry[act] = E[act][:, None] * sol[n:] / c
    return (Rw[:, 0], Ry[:, 0]) if one else (Rw, Ry)


def raw_gradients(r_w, r_y, low, upp):
    """(d_q, d_l, d_u) in the convention of include/mpcqp_adjoint.h: a lower-active or equality row has r_y in d_l, an upper-active one in d_u."""
    low = low.reshape(low.shape + (1,) * (np.ndim(r_y) - 1))
    upp = upp.reshape(low.shape)
    return -r_w, np.where(low, r_y, 0.0), np.where(upp, r_y, 0.0)


def parameter_maps(kw, attrs=None):
    """Jacobians of (q, l, u) with respect to (x0, uminus1, xref, uref), read off the host QP builder: dict name -> (Jq [n, p], Jl [m, p],
    Ju [m, p]).  kw: constructor kwargs of the controller; xref in the shape it is used in ((nx,) or (Np+1, nx): p = its size)."""
    from pympc_amd import MPCController
    kw = dict(kw)
    nx, nu = np.asarray(kw['Bd']).shape
    kw.setdefault('x0', np.zeros(nx)); kw.setdefault('uref', np.zeros(nu)); kw.setdefault('xref', np.zeros(nx))
    kw.setdefault('uminus1', np.array(kw['uref'], dtype=float))

    def vectors(over):
        k2 = dict(kw); k2.update(over)
        K = MPCController(**k2)
        for a, v in (attrs or {}).items():
            setattr(K, a, v)
        K.x0_rh, K.uminus1_rh = np.copy(K.x0), np.copy(K.uminus1)
        K._compute_QP_matrices_()
        return np.array(K._q, dtype=float), np.array(K._l, dtype=float), np.array(K._u, dtype=float)

    q0, l0, u0 = vectors({})
    def diff(a, b):                                        # (infinite bounds do not move)
        with np.errstate(invalid='ignore'):
            return np.where(np.isfinite(a) & np.isfinite(b), a - b, 0.0)
    maps = {}
    for name in ('x0', 'uminus1', 'xref', 'uref'):
        base = np.array(kw[name], dtype=float)
        cols = []
        for j in range(base.size):
            v = base.copy().ravel(); v[j] += 1.0
            q1, l1, u1 = vectors({name: v.reshape(base.shape)})
            cols.append((diff(q1, q0), diff(l1, l0), diff(u1, u0)))
        maps[name] = tuple(np.stack([c[i] for c in cols], axis=1) for i in range(3))
    return maps


def chain(maps, d_q, d_l, d_u):
    """dL/d(parameter) = Jq' d_q + Jl' d_l + Ju' d_u.  (An equality row moves both its bounds; by the convention of raw_gradients its
    derivative with respect to the common value is in d_l and d_u is 0 there, so it is counted once.)"""
    return {name: Jq.T @ d_q + Jl.T @ d_l + Ju.T @ d_u for name, (Jq, Jl, Ju) in maps.items()}


def adjoint(P, A, l, u, x, z, y, D, E, c, G, maps=None, weak_tol=WEAK_TOL):
    """Everything mpcqp_adjoint returns for the seeds G [n] or [n, k], from the iterate (x, z, y) and the scaling (D, E, c): dict with
    r_w, r_y, d_q, d_l, d_u, low, upp, n_active, n_weak and, with `maps` (parameter_maps), x0 / uminus1 / xref / uref."""
    low, upp = active_rows(A, l, u, x, z, y, D, E, c)
    r_w, r_y = solve_adjoint(P, A, low, upp, G, D, E, c)
    d_q, d_l, d_u = raw_gradients(r_w, r_y, low, upp)
    res = dict(r_w=r_w, r_y=r_y, d_q=d_q, d_l=d_l, d_u=d_u, low=low, upp=upp, n_active=int(np.count_nonzero(low | upp)),
               n_weak=count_weak(l, u, z, y, weak_tol))
    if maps is not None:
        res.update(chain(maps, d_q, d_l, d_u))
    return res


def gains(P, A, l, u, x, z, y, D, E, c, maps, ou, nu):
    """The Jacobians of u_0: dict K_x0 [nu, nx], K_um1 [nu, nu], K_xref [nu, p], K_uref [nu, nu] (+ n_active, n_weak): the nu unit seeds
    of the u_0 block (variables ou .. ou + nu - 1)."""
    n = sp.csc_matrix(P).shape[0]
    G = np.zeros((n, nu)); G[ou + np.arange(nu), np.arange(nu)] = 1.0
    r = adjoint(P, A, l, u, x, z, y, D, E, c, G, maps)
    return dict(K_x0=r['x0'].T, K_um1=r['uminus1'].T, K_xref=r['xref'].T, K_uref=r['uref'].T, n_active=r['n_active'], n_weak=r['n_weak'],
                low=r['low'], upp=r['upp'])
