"""Restatement of the model gradients of the adjoint (include/mpcqp_adjoint_model.h) for the tests: numpy only, sharing nothing with the
HIP kernel (pympc_amd/csrc/mpcqp_adjoint_model.h).

For a seed g = dL/dw, with [r_w; r_y] from tests/adjoint_ref.py and the solution (w, y), a perturbation of the problem data moves the loss by
    dL = -r_w' (dP w + dq + dA' y) + r_y' (db - dA w).
``builder_gradients`` writes no chain rule down: P, q, A, l, u are affine in every entry of Ad, Bd, Qx, QxN, Qu, QDu and in eps_feas, so their
Jacobians are read off the host builder itself (MPCController._compute_QP_matrices_, i.e. pympc_amd/qp_build.py) by moving one entry at a
time by one unit -- a weight's entries (i, j) and (j, i) together, the weights being symmetric: the gradient with respect to a symmetric
perturbation, dL = <d_Q, dQ>, so a pair's dL is 2 d_Q[i, j].  ``closed_form`` holds the sums of the header as a second, independent
function, with the sum of the absolute values of each entry's terms beside it (what a rounding bound scales with).
"""
import numpy as np

NAMES = ('Ad', 'Bd', 'Qx', 'QxN', 'Qu', 'QDu', 'eps_feas')
WEIGHTS = ('Qx', 'QxN', 'Qu', 'QDu')


def full_kwargs(kw):
    """Constructor kwargs with every default the gradients are taken against spelled out (QxN no longer aliases Qx, uminus1 not uref)."""
    kw2 = dict(kw)
    nx, nu = np.asarray(kw2['Bd']).shape
    kw2['Ad'], kw2['Bd'] = np.array(kw2['Ad'], dtype=float), np.array(kw2['Bd'], dtype=float)
    for k, shape in (('Qx', (nx, nx)), ('Qu', (nu, nu)), ('QDu', (nu, nu))):
        kw2[k] = np.zeros(shape) if kw2.get(k) is None else np.array(kw2[k], dtype=float)
    kw2['QxN'] = kw2['Qx'].copy() if kw2.get('QxN') is None else np.array(kw2['QxN'], dtype=float)
    kw2['x0'] = np.zeros(nx) if kw2.get('x0') is None else np.array(kw2['x0'], dtype=float)
    kw2['uref'] = np.zeros(nu) if kw2.get('uref') is None else np.array(kw2['uref'], dtype=float)
    kw2['xref'] = np.zeros(nx) if kw2.get('xref') is None else np.array(kw2['xref'], dtype=float)
    kw2['uminus1'] = kw2['uref'].copy() if kw2.get('uminus1') is None else np.array(kw2['uminus1'], dtype=float)
    kw2.setdefault('eps_feas', 1e6)
    kw2['eps_feas'] = float(kw2['eps_feas'])
    return kw2


def build(kw, attrs=None):
    """(P [n, n], q, A [m, n], l, u) dense, of the host builder for these kwargs and attribute switches, and the controller."""
    from pympc_amd import MPCController
    K = MPCController(**kw)
    for a, v in (attrs or {}).items():
        setattr(K, a, v)
    K.x0_rh, K.uminus1_rh = np.copy(K.x0), np.copy(K.uminus1)
    K._compute_QP_matrices_()
    return (K.P.toarray(), np.array(K._q, dtype=float), K.A.toarray(), np.array(K._l, dtype=float), np.array(K._u, dtype=float)), K


def _entries(name, shape):
    """The unit perturbations of one matrix: (i, j) for Ad, Bd; the pairs i <= j for a weight."""
    if name in WEIGHTS:
        return [(i, j) for i in range(shape[0]) for j in range(i, shape[1])]
    return [(i, j) for i in range(shape[0]) for j in range(shape[1])]


def perturbed(kw, name, i, j, step):
    """kwargs with entry (i, j) of ``name`` moved by ``step`` (a weight: (j, i) with it; eps_feas: the scalar)."""
    k2 = dict(kw)
    if name == 'eps_feas':
        k2['eps_feas'] = kw['eps_feas'] + step
        return k2
    M = np.array(kw[name], dtype=float)
    M[i, j] += step
    if name in WEIGHTS and i != j:
        M[j, i] += step
    k2[name] = M
    return k2


def _fin_diff(a, b):
    with np.errstate(invalid='ignore'):
        return np.where(np.isfinite(a) & np.isfinite(b), a - b, 0.0)


def builder_gradients(kw, attrs, w, y, r_w, r_y, low, upp):
    """dict name -> gradient, and name -> sum of |terms| per entry, from unit perturbations of the host builder and the dL formula.
    kw: full_kwargs(...).  low / upp: the active masks (db moves d_l on a lower-active or equality row, d_u on an upper-active one)."""
    (P0, q0, A0, l0, u0), _ = build(kw, attrs)
    nx, nu = kw['Bd'].shape
    shapes = dict(Ad=(nx, nx), Bd=(nx, nu), Qx=(nx, nx), QxN=(nx, nx), Qu=(nu, nu), QDu=(nu, nu))
    d_l, d_u = np.where(low, r_y, 0.0), np.where(upp, r_y, 0.0)
    grads, mags = {}, {}

    def dL(over):
        (P1, q1, A1, l1, u1), _ = build(over, attrs)
        dP, dq, dA = P1 - P0, q1 - q0, A1 - A0
        dl, du = _fin_diff(l1, l0), _fin_diff(u1, u0)
        terms = [-(r_w[:, None] * dP * w[None, :]), -(r_w * dq), -(y[:, None] * dA * r_w[None, :]), -(r_y[:, None] * dA * w[None, :]), d_l * dl, d_u * du]
        return sum(t.sum() for t in terms), sum(np.abs(t).sum() for t in terms)

    for name in NAMES[:6]:
        G, M = np.zeros(shapes[name]), np.zeros(shapes[name])
        for i, j in _entries(name, shapes[name]):
            v, mag = dL(perturbed(kw, name, i, j, 1.0))
            if name in WEIGHTS and i != j:
                G[i, j] = G[j, i] = 0.5 * v
                M[i, j] = M[j, i] = 0.5 * mag
            else:
                G[i, j], M[i, j] = v, mag
        grads[name], mags[name] = G, M
    v, mag = dL(perturbed(kw, 'eps_feas', 0, 0, 1.0))
    grads['eps_feas'], mags['eps_feas'] = np.float64(v), np.float64(mag)
    return grads, mags


def closed_form(nx, nu, Np, Nc, soft, w, y, r_w, r_y, xref, uref, uminus1, on=(True, True, True)):
    """The sums of include/mpcqp_adjoint_model.h: dict name -> gradient, dict name -> sum of |terms| per entry.  xref: (nx,) or (Np+1, nx);
    on = (JX_ON, JU_ON, JDU_ON): a weight whose cost term the controller runs without gets zero."""
    N = Np + 1
    n_x, n_u = N * nx, Nc * nu
    X, RX = w[:n_x].reshape(N, nx), r_w[:n_x].reshape(N, nx)
    U, RU = w[n_x:n_x + n_u].reshape(Nc, nu), r_w[n_x:n_x + n_u].reshape(Nc, nu)
    Y, RY = y[:n_x].reshape(N, nx), r_y[:n_x].reshape(N, nx)
    XR = np.broadcast_to(np.asarray(xref, dtype=float).reshape(-1, nx)[:N] if np.ndim(xref) == 2 else np.asarray(xref, dtype=float), (N, nx))
    sym = lambda M: 0.5 * (M + M.T)
    out = lambda a, b: np.multiply.outer(a, b)
    g = {k: np.zeros(s) for k, s in (('Ad', (nx, nx)), ('Bd', (nx, nu)), ('Qx', (nx, nx)), ('QxN', (nx, nx)), ('Qu', (nu, nu)), ('QDu', (nu, nu)))}
    a = {k: np.zeros_like(v) for k, v in g.items()}

    def add(name, M, weight_term):
        if weight_term:
            g[name] -= sym(M); a[name] += 0.5 * (np.abs(M) + np.abs(M.T))
        else:
            g[name] -= M; a[name] += np.abs(M)

    for k in range(Np):
        ku = min(k, Nc - 1)
        add('Ad', out(Y[k + 1], RX[k]), False); add('Ad', out(RY[k + 1], X[k]), False)
        add('Bd', out(Y[k + 1], RU[ku]), False); add('Bd', out(RY[k + 1], U[ku]), False)
        if on[0]:
            add('Qx', out(RX[k], X[k]), True); add('Qx', -out(RX[k], XR[k]), True)
    if on[0]:
        add('QxN', out(RX[Np], X[Np]), True); add('QxN', -out(RX[Np], XR[Np]), True)
    for k in range(Nc):
        iu = float(Np - Nc + 1) if k == Nc - 1 else 1.0
        if on[1]:
            add('Qu', iu * out(RU[k], U[k]), True); add('Qu', -iu * out(RU[k], uref), True)
        if on[2]:
            dr = RU[k] - (RU[k - 1] if k > 0 else 0.0)
            du = U[k] - (U[k - 1] if k > 0 else np.asarray(uminus1, dtype=float))
            add('QDu', out(dr, du), True)
    if soft:
        t = r_w[n_x + n_u:] * w[n_x + n_u:]
        g['eps_feas'], a['eps_feas'] = np.float64(-t.sum()), np.float64(np.abs(t).sum())
    else:
        g['eps_feas'], a['eps_feas'] = np.float64(0.0), np.float64(0.0)
    return g, a


def closed_form_of(kw, attrs, w, y, r_w, r_y):
    """closed_form for a controller given by full_kwargs(...) and its attribute switches."""
    attrs = attrs or {}
    nx, nu = kw['Bd'].shape
    Np = kw['Np']
    Nc = Np if kw.get('Nc') is None else kw['Nc']
    on = (attrs.get('JX_ON', True), attrs.get('JU_ON', True), attrs.get('JDU_ON', True))
    return closed_form(nx, nu, Np, Nc, attrs.get('SOFT_ON', True), w, y, r_w, r_y, kw['xref'], kw['uref'], kw['uminus1'], on)
