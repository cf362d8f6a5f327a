"""What the Riccati tests share (tests/test_riccati_ref.py, tests/test_gpu_riccati.py): a numpy restatement of the two kernels of
pympc_amd/csrc/mpcqp_riccati.hip -- the structure-preserving doubling algorithm for the discrete algebraic Riccati equation and the adjoint
of its solution and gain (include/mpcqp_riccati.h) --, the case list, the scipy reference, finite differences of it,
and the bounds the device is held to.  The restatement follows the kernels step by step (same stopping rule, same statuses), in numpy's
own summation order."""
import numpy as np
import scipy.linalg as sla

from pympc_amd import fixtures

MAX_ITER, TOL = 50, 1e-15
sym = lambda M: 0.5 * (M + M.T)
amax = lambda M: float(np.abs(M).max()) if np.size(M) else 0.0


def _chol(M):
    """Lower Cholesky factor, or the status of the refusal: -1 for a pivot <= 0, 0 for one that is not a number."""
    if not np.all(np.isfinite(M)):
        return None, 0
    try:
        return np.linalg.cholesky(M), 1
    except np.linalg.LinAlgError:
        return None, -1


def dare(A, B, Q, R, gain_form=0, max_iter=MAX_ITER, tol=TOL):
    """(X, gain, status, iters, res) of one instance, as mpcqp_dare writes them."""
    A, B, Q, R = (np.atleast_2d(np.asarray(M, dtype=float)) for M in (A, B, Q, R))
    n, m = B.shape
    zero = (np.zeros((n, n)), np.zeros((m, n)), 0, 0, 0.0)
    Lr, st = _chol(R)
    if st != 1:
        return zero[:2] + (st, 0, 0.0)
    Y = sla.solve_triangular(Lr, B.T, lower=True)
    G, H, Ak = Y.T @ Y, Q.copy(), A.copy()
    it, done = 0, False
    with np.errstate(all='ignore'):
        while it < max_iter and not done:
            W = np.eye(n) + G @ H
            try:
                Z = np.linalg.solve(W, np.hstack([Ak, G]))
            except np.linalg.LinAlgError:
                Z = np.full((n, 2 * n), np.nan)
            Z1, Z2 = Z[:, :n], Z[:, n:]
            dG, dH, An = sym((Ak @ Z2) @ Ak.T), sym(Ak.T @ (H @ Z1)), Ak @ Z1
            G, H, Ak = G + dG, H + dH, An
            it += 1
            if not (np.isfinite(amax(dH)) and np.isfinite(amax(H)) and np.isfinite(amax(G)) and np.isfinite(amax(Ak))):
                return zero[:2] + (0, it, 0.0)
            done = amax(dH) <= tol * max(1.0, amax(H))
    if not done:
        return zero[:2] + (0, it, 0.0)
    X = H
    XB, XA = X @ B, X @ A
    M, P = R + sym(B.T @ XB), B.T @ XA
    Lm, st = _chol(M)
    if st != 1:
        return zero[:2] + (st, it, 0.0)
    K0 = sla.cho_solve((Lm, True), P)
    gain = K0 if gain_form == 0 else sla.cho_solve((Lm, True), XB.T)
    res = amax(X - (A.T @ XA - P.T @ K0 + Q)) / max(1.0, amax(X))
    if not np.isfinite(res):
        return zero[:2] + (0, it, 0.0)
    return X, gain, 1, it, res


def dare_adjoint(A, B, Q, R, X, K, G_X=None, G_K=None, gain_form=0, max_iter=MAX_ITER, tol=TOL):
    """(d_A, d_B, d_Q, d_R, iters) of one converged instance, as mpcqp_dare_adjoint writes them (``K``: the gain in the form asked for)."""
    A, B, Q, R, X, K = (np.atleast_2d(np.asarray(M, dtype=float)) for M in (A, B, Q, R, X, K))
    n, m = B.shape
    G_X = np.zeros((n, n)) if G_X is None else np.asarray(G_X, dtype=float).reshape(n, n)
    G_K = np.zeros((m, n)) if G_K is None else np.asarray(G_K, dtype=float).reshape(m, n)
    XB = X @ B
    M = R + sym(B.T @ XB)
    K0 = K if gain_form == 0 else K @ A
    Acl = A - B @ K0
    T = sla.cho_solve((np.linalg.cholesky(M), True), G_K)
    Mb = -T @ K.T
    if gain_form == 0:
        Xb = sym(G_X + B @ T @ A.T + B @ Mb @ B.T)
    else:
        Xb = sym(G_X + sym(B @ T) + B @ sym(Mb) @ B.T)
    Lam, S, it, done = Xb.copy(), Acl.copy(), 0, False
    while it < max_iter and not done:
        dL = sym(S @ Lam @ S.T)
        Lam, S = Lam + dL, S @ S
        it += 1
        done = amax(dL) <= tol * max(1.0, amax(Lam))
    assert done
    XAL = X @ Acl @ Lam
    d_Q = Lam
    d_R = sym(Mb) + sym(K0 @ Lam @ K0.T)
    if gain_form == 0:
        d_A = XB @ T + 2 * XAL
        d_B = X @ A @ T.T + XB @ (Mb + Mb.T) - 2 * XAL @ K0.T
    else:
        d_A = 2 * XAL
        d_B = X @ T.T + XB @ (Mb + Mb.T) - 2 * XAL @ K0.T
    return d_A, d_B, d_Q, d_R, it


# ---- the scipy reference ---------------------------------------------------------------------------------------------------------------
def scipy_dare(A, B, Q, R, gain_form=0):
    X = sla.solve_discrete_are(A, B, Q, R)
    M = R + B.T @ X @ B
    return X, np.linalg.solve(M, B.T @ X @ (A if gain_form == 0 else np.eye(A.shape[0])))


def fd_loss_gradients(A, B, Q, R, G_X, G_K, gain_form, solve=scipy_dare, h=1e-6):
    """Central differences of <G_X, X> + <G_K, gain> in every entry of A and B and in every symmetric direction of Q and R (the gradient of
    a symmetric perturbation, as d_Q and d_R are defined)."""
    def loss(A, B, Q, R):
        X, K = solve(A, B, Q, R, gain_form)
        return float((G_X * X).sum() + (G_K * K).sum())
    out = []
    for idx, M in enumerate((A, B, Q, R)):
        g = np.zeros_like(M)
        symmetric = idx >= 2
        for i in range(M.shape[0]):
            for j in range(i if symmetric else 0, M.shape[1]):
                E = np.zeros_like(M)
                E[i, j] = 1.0
                if symmetric:
                    E[j, i] = 1.0
                args = lambda s: [a + s * h * E if k == idx else a for k, a in enumerate((A, B, Q, R))]
                d = (loss(*args(1.0)) - loss(*args(-1.0))) / (2 * h)
                if symmetric and i != j:
                    g[i, j] = g[j, i] = d / 2          # <d_Q, E> = d_Q[i,j] + d_Q[j,i]
                else:
                    g[i, j] = d
        out.append(g)
    return out


def fd_directional(A, B, Q, R, G_X, G_K, gain_form, grads, ndir=3, solve=scipy_dare, h=1e-6, seed=0):
    """The largest |<grad, D> - central difference along D| / (|grad|_F |D|_F) over ``ndir`` random unit directions D in each of A, B, Q, R
    (symmetric ones for Q and R): what a comparison of every entry measures, at a cost that does not grow with the size."""
    rng = np.random.default_rng(seed)
    loss = lambda P: (lambda X, K: float((G_X * X).sum() + (G_K * K).sum()))(*solve(*P, gain_form))
    worst, P0 = 0.0, (A, B, Q, R)
    for idx, M in enumerate(P0):
        for _ in range(ndir):
            D = rng.standard_normal(M.shape)
            D = (sym(D) if idx >= 2 else D)
            D /= np.linalg.norm(D)
            Pp = [a + h * D if k == idx else a for k, a in enumerate(P0)]
            Pm = [a - h * D if k == idx else a for k, a in enumerate(P0)]
            fd = (loss(Pp) - loss(Pm)) / (2 * h)
            worst = max(worst, abs(float((grads[idx] * D).sum()) - fd) / max(np.linalg.norm(grads[idx]), 1e-300))
    return worst


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def _spd(rng, k, lo=0.5):
    M = rng.standard_normal((k, k))
    return M @ M.T / k + lo * np.eye(k)


def _random(seed, n, m, rho):
    rng = np.random.default_rng(7000 + seed)
    G = rng.standard_normal((n, n))
    A = G * (rho / np.max(np.abs(np.linalg.eigvals(G))))
    return A, rng.standard_normal((n, m)), _spd(rng, n), _spd(rng, m)


def _fixture(name, R='Qu', **kw):
    f = fixtures.NAMED[name]() if not kw else getattr(fixtures, name)(**kw)
    return f['Ad'], f['Bd'], f['Qx'], f[R]


def _kalman_dual(name):
    f = fixtures.NAMED[name]()
    C = np.array([[1.0, 0, 0, 0], [0, 0, 1.0, 0]])
    return f['Ad'].T.copy(), C.T.copy(), np.diag([0.1, 10, 0.1, 10]) * 1e-2, 0.01 * np.eye(2)


SCALAR = (np.array([[1.1]]), np.array([[0.7]]), np.array([[2.0]]), np.array([[0.3]]))


def scalar_root(a, b, q, r):
    """The positive root of b^2 X^2 + (r - a^2 r - q b^2) X - q r = 0."""
    c1 = r - a * a * r - q * b * b
    return (-c1 + np.sqrt(c1 * c1 + 4 * b * b * q * r)) / (2 * b * b)


CASES = {
    'scalar': lambda: SCALAR,
    'point_mass': lambda: _fixture('point_mass'),
    'accel_brake': lambda: _fixture('accel_brake'),
    'small_mimo': lambda: _fixture('small_mimo'),
    'random_3_5': lambda: _random(0, 3, 5, 1.1),
    'cart_pole': lambda: _fixture('cart_pole', R='QDu'),
    'cart_pole_5ms': lambda: _fixture('cart_pole_kalman', R='QDu'),
    'kalman_dual_cart_pole': lambda: _kalman_dual('cart_pole'),
    'kalman_dual_cart_pole_5ms': lambda: _kalman_dual('cart_pole_kalman'),
    'random_5_3': lambda: _random(1, 5, 3, 0.9),
    'quadcopter': lambda: _fixture('quadcopter'),
    'random_lti_0': lambda: _fixture('random_lti', index=0),
    'random_17_3': lambda: _random(2, 17, 3, 0.95),
    'random_lti_20_8': lambda: _fixture('random_lti', index=1, nx=20, nu=8),
    'random_32_8': lambda: _random(3, 32, 8, 1.0),
    'random_32_32': lambda: _random(4, 32, 32, 1.05),
}
NOT_PD = 'cart_pole_qu0'                    # cart_pole with its own Qu = 0: status -1
SMALL_FD = ('point_mass', 'small_mimo')     # where the device is also compared with central differences through its own forward


def case(name):
    if name == NOT_PD:
        return _fixture('cart_pole')
    return tuple(np.array(M, dtype=float) for M in CASES[name]())


def copies(name, B=3):
    """The case and B - 1 perturbed copies of it (entries of A and B scaled by 1 + 0.01 u, u uniform in [-1, 1]: zeros stay zeros)."""
    A, Bm, Q, R = case(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    out = [(A, Bm, Q, R)]
    for _ in range(B - 1):
        out.append((A * (1 + 0.01 * rng.uniform(-1, 1, A.shape)), Bm * (1 + 0.01 * rng.uniform(-1, 1, Bm.shape)), Q, R))
    return out


def seeds(name, n, m):
    rng = np.random.default_rng(31 + sum(map(ord, name)))
    return sym(rng.standard_normal((n, n))), rng.standard_normal((m, n))


def rel(a, b):
    """|a - b|_max relative to |b|_max."""
    return amax(np.asarray(a) - np.asarray(b)) / max(amax(b), 1e-300)


# ---- the bounds --------------------------------------------------------------------------------------------------------------------------
# E_REF[case] = (X, gain form 0, gain form 1): the restatement's distance from scipy, relative to |X|_max / |gain|_max, the largest over
# copies(case); RES_REF: its residual; E_REF_ADJ: the largest relative distance of its adjoint from central differences of scipy over
# d_A, d_B, d_Q, d_R and both gain forms (fd_directional: along random directions, relative to the gradient's norm).  Measured with
# tests/test_riccati_ref.py -s; LAB_NOTES.md has the device's own figures beside them.
FACTOR, FLOOR, RES_FLOOR, FD_BOUND = 100.0, 1e-13, 1e-14, 1e-5
# (measured 2026-10-19)
E_REF = {
    'scalar': (3.4e-16, 1.8e-16, 1.9e-16), 'point_mass': (4.5e-14, 4e-14, 4e-14), 'accel_brake': (2.1e-15, 1.9e-15, 1.9e-15),
    'small_mimo': (1.9e-15, 3.5e-15, 3.9e-15), 'random_3_5': (9.5e-16, 1.8e-15, 1.1e-15), 'cart_pole': (2e-14, 9.1e-15, 9e-15),
    'cart_pole_5ms': (1.9e-12, 1.8e-12, 1.8e-12), 'kalman_dual_cart_pole': (8.4e-15, 4.5e-15, 5.1e-15),
    'kalman_dual_cart_pole_5ms': (1.7e-14, 1.6e-14, 1.7e-14), 'random_5_3': (8e-16, 1e-15, 1.1e-15), 'quadcopter': (2e-14, 1.1e-14, 1.6e-14),
    'random_lti_0': (4.9e-15, 2.4e-15, 2.6e-15), 'random_17_3': (1e-14, 6.3e-15, 7.7e-15), 'random_lti_20_8': (2e-14, 1.6e-14, 2.1e-14),
    'random_32_8': (7e-15, 8e-15, 7.2e-15), 'random_32_32': (2.4e-15, 1.2e-14, 8.4e-15)}
RES_REF = {
    'scalar': 3.4e-16, 'point_mass': 2.9e-16, 'accel_brake': 1.5e-16, 'small_mimo': 1.9e-16, 'random_3_5': 3.8e-16, 'cart_pole': 1.1e-15,
    'cart_pole_5ms': 2.1e-16, 'kalman_dual_cart_pole': 2.2e-16, 'kalman_dual_cart_pole_5ms': 3.5e-16, 'random_5_3': 1.3e-16,
    'quadcopter': 4.3e-16, 'random_lti_0': 5.1e-15, 'random_17_3': 4.9e-15, 'random_lti_20_8': 2.3e-14, 'random_32_8': 6e-15,
    'random_32_32': 2.1e-15}
E_REF_ADJ = {
    'scalar': 3.4e-10, 'point_mass': 1.3e-07, 'accel_brake': 1.8e-08, 'small_mimo': 1.1e-08, 'random_3_5': 1.4e-09, 'cart_pole': 2.5e-09,
    'cart_pole_5ms': 1.6e-08, 'kalman_dual_cart_pole': 2.8e-09, 'kalman_dual_cart_pole_5ms': 5.4e-09, 'random_5_3': 2.6e-08,
    'quadcopter': 5.9e-09, 'random_lti_0': 3e-08, 'random_17_3': 2.5e-07, 'random_lti_20_8': 7.9e-08, 'random_32_8': 1.5e-07,
    'random_32_32': 2.5e-08}


def bound(name, which):
    """The device's bound against scipy for X (which = 0) or the gain in form which - 1."""
    return max(FACTOR * E_REF[name][which], FLOOR)


def res_bound(name):
    return max(FACTOR * RES_REF[name], RES_FLOOR)


def adj_bound(name):
    return max(FACTOR * E_REF_ADJ[name], FLOOR)
