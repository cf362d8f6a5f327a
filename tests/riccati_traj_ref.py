"""What the tests of the Riccati difference equation share (tests/test_riccati_traj_ref.py, tests/test_gpu_riccati_traj.py): the recursion of
include_ext3/mpcqp_riccati_traj.h in two forms on the CPU (torch, float64), its gradients by autograd, the designs made of it, the case
list and the bounds the device is held to.  Nothing here comes from the device.

    form one   S = R + B'XB,  K = S^-1 B'XA,  F = S^-1 B'X,  X+ = sym(A'XA - A'XB K + Q)           (the form of the header)
    form two   X+ = sym(Acl'X Acl + K'RK + Q),  Acl = A - B K                                       (the Joseph form: another rounding path)

Every array is batched: A is [T, Bt, n, n] (a trajectory) or [Bt, n, n] (one matrix per instance), B likewise, Q, R, X0 are [Bt, ., .]."""
import contextlib
import functools

import numpy as np
import torch

import riccati_ref as rr

_sym = lambda M: 0.5 * (M + M.transpose(-1, -2))
_T = lambda M: M.transpose(-1, -2)


def recursion(A, B, Q, R, X0, T, form=1):
    """(X [T+1, Bt, n, n], K [T, Bt, m, n], F [T, Bt, m, n]) of torch tensors; differentiable."""
    X, Xs, Ks, Fs = _sym(X0), [], [], []
    Xs.append(X)
    for t in range(T):
        At, Bt = (A[t] if A.dim() == 4 else A), (B[t] if B.dim() == 4 else B)
        S = R + _T(Bt) @ X @ Bt
        BtX = _T(Bt) @ X
        K, F = torch.linalg.solve(S, BtX @ At), torch.linalg.solve(S, BtX)
        if form == 1:
            X = _sym(_T(At) @ X @ At - _T(At) @ X @ Bt @ K + Q)
        else:
            Acl = At - Bt @ K
            X = _sym(_T(Acl) @ X @ Acl + _T(K) @ R @ K + Q)
        Xs.append(X); Ks.append(K); Fs.append(F)
    return torch.stack(Xs), torch.stack(Ks), torch.stack(Fs)


_NAMES = ('A', 'B', 'Q', 'R', 'X0')


@contextlib.contextmanager
def _one_thread():
    """These matrices are tiny: torch's thread pool costs a hundred times what it saves (put back afterwards)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)
_tt = lambda a, grad=False: torch.tensor(np.asarray(a, dtype=float), dtype=torch.float64, requires_grad=grad)


def run(mats, T, form=1):
    """The same for a dict of numpy arrays by the names A, B, Q, R, X0: numpy arrays back."""
    with torch.no_grad(), _one_thread():
        return tuple(o.numpy() for o in recursion(*(_tt(mats[k]) for k in _NAMES), T, form))


def gradients(mats, T, G_X=None, G_K=None, gain_form=0, form=1):
    """The gradients of sum_t <G_X[t], X_t> + sum_t <G_K[t], gain_t> by autograd, a dict by the names A, B, Q, R, X0 of numpy arrays shaped
    like the inputs; those of Q, R and X0 symmetrized (the gradient of a symmetric perturbation)."""
    P = [_tt(mats[k], True) for k in _NAMES]
    with _one_thread():
        X, K, F = recursion(*P, T, form)
        loss = 0.0
        if G_X is not None:
            loss = loss + (_tt(G_X) * X).sum()
        if G_K is not None:
            loss = loss + (_tt(G_K) * (K if gain_form == 0 else F)).sum()
        g = [torch.zeros_like(p) if v is None else v for p, v in zip(P, torch.autograd.grad(loss, P, allow_unused=True))]
    return {k: (_sym(v) if k in ('Q', 'R', 'X0') else v).numpy() for k, v in zip(_NAMES, g)}


def fd_directional(mats, T, G_X, G_K, gain_form, grads, ndir=3, h=1e-6, seed=0):
    """riccati_ref.fd_directional's scheme on the recursion: the largest |<grad, D> - central difference along D| / |grad|_F over ``ndir`` random
    unit directions D in each of A, B, Q, R, X0 (symmetric ones for Q, R, X0)."""
    rng = np.random.default_rng(seed)

    def loss(M):
        X, K, F = run(M, T)
        return float((G_X * X).sum() + (G_K * (K if gain_form == 0 else F)).sum())
    worst = 0.0
    for k in _NAMES:
        for _ in range(ndir):
            D = rng.standard_normal(mats[k].shape)
            D = 0.5 * (D + np.swapaxes(D, -1, -2)) if k in ('Q', 'R', 'X0') else D
            D /= np.linalg.norm(D)
            fd = (loss(dict(mats, **{k: mats[k] + h * D})) - loss(dict(mats, **{k: mats[k] - h * D}))) / (2 * h)
            worst = max(worst, abs(float((grads[k] * D).sum()) - fd) / max(np.linalg.norm(grads[k]), 1e-300))
    return worst


# ---- the designs ---------------------------------------------------------------------------------------------------------------------------
def kalman_gain_traj(A_traj, C, Qn, Rn, P0, hold=1):
    """(L_traj [nentries, Bt, nx, ny], P_traj [nentries + 1, Bt, nx, nx]) by the dual mapping: entry e = the gain and the covariance at step e hold."""
    A_traj = np.asarray(A_traj, dtype=float)
    nent, Bt = A_traj.shape[:2]
    rep = np.repeat(np.swapaxes(A_traj, -1, -2), hold, axis=0)
    bc = lambda M: np.broadcast_to(np.asarray(M, dtype=float), (Bt,) + np.shape(M)[-2:])
    X, _, F = run(dict(A=rep, B=np.swapaxes(bc(C), -1, -2), Q=bc(Qn), R=bc(Rn), X0=bc(P0)), nent * hold)
    return np.swapaxes(F[::hold], -1, -2), X[::hold]


def lqr_traj(Ad_traj, Bd_traj, Qx, Qu, QxN):
    """(P_traj [T + 1, Bt, n, n], K_traj [T, Bt, m, n]) in forward time order: the recursion on the reversed schedule from QxN."""
    Ad_traj, Bd_traj = np.asarray(Ad_traj, dtype=float), np.asarray(Bd_traj, dtype=float)
    T, Bt = Ad_traj.shape[:2]
    bc = lambda M: np.broadcast_to(np.asarray(M, dtype=float), (Bt,) + np.shape(M)[-2:])
    X, K, _ = run(dict(A=Ad_traj[::-1].copy(), B=Bd_traj[::-1].copy(), Q=bc(Qx), R=bc(Qu), X0=bc(QxN)), T)
    return X[::-1].copy(), K[::-1].copy()


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
CASES = ('scalar', 'random_3_5', 'random_5_3', 'kalman_dual_cart_pole', 'random_17_3', 'random_32_32')
STEPS = (1, 2, 7)
PATTERNS = ('A', 'B', 'AB', 'none')        # which of A and B is a trajectory
BATCH = 3


def initial(name, n):
    """A symmetric positive definite X0 for the case."""
    return rr._spd(np.random.default_rng(77 + sum(map(ord, name))), n, lo=0.1)


@functools.lru_cache(maxsize=None)
def _make(name, T, pattern):
    insts = rr.copies(name, BATCH)
    n, m = insts[0][1].shape
    rng = np.random.default_rng(1000 * T + sum(map(ord, name + pattern)))
    step = lambda M: np.stack([np.stack([i[M] * (1 + 0.01 * rng.uniform(-1, 1, i[M].shape)) for i in insts]) for _ in range(T)])      # (zeros stay zeros)
    mats = dict(A=step(0) if 'A' in pattern else np.stack([i[0] for i in insts]), B=step(1) if 'B' in pattern else np.stack([i[1] for i in insts]),
                Q=np.stack([i[2] for i in insts]), R=np.stack([i[3] for i in insts]), X0=np.stack([initial(name, n) * (1 + 0.1 * b) for b in range(BATCH)]))
    for v in mats.values():
        v.setflags(write=False)
    return mats


def make(name, T, pattern):
    """The case as a dict of read-only arrays: BATCH perturbed copies (riccati_ref.copies), and per step of a trajectory another perturbation
    of the same kind (entries scaled by 1 + 0.01 u)."""
    return dict(_make(name, T, pattern))


def seeds(name, T, n, m):
    rng = np.random.default_rng(53 + T + sum(map(ord, name)))
    G = rng.standard_normal((T + 1, BATCH, n, n))
    return 0.5 * (G + np.swapaxes(G, -1, -2)), rng.standard_normal((T, BATCH, m, n))


def rel(a, b):
    """riccati_ref.rel per instance (axis -3 is the batch), the largest."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim == 4:
        return max(rr.rel(a[:, i], b[:, i]) for i in range(a.shape[1]))
    return max(rr.rel(a[i], b[i]) for i in range(a.shape[0]))


# ---- the bounds --------------------------------------------------------------------------------------------------------------------------
# E_REF_TRAJ[case]: the largest relative distance (rel) between the two forms over X_traj and both gains, over STEPS and PATTERNS;
# E_REF_TRAJ_ADJ[case]: the same between autograd through form one and autograd through form two, over every gradient, the seeds on X, on
# either gain and on both.  Measured with tests/test_riccati_traj_ref.py -s.  The device is held to max(FACTOR x, FLOOR) of riccati_ref.
# (measured 2026-10-20)
E_REF_TRAJ = {
    'scalar': 3.5e-16, 'random_3_5': 2.0e-15, 'random_5_3': 1.5e-15, 'kalman_dual_cart_pole': 1.8e-14, 'random_17_3': 6.2e-16, 'random_32_32': 1.4e-14}
E_REF_TRAJ_ADJ = {
    'scalar': 5.9e-14, 'random_3_5': 3.9e-14, 'random_5_3': 8.9e-15, 'kalman_dual_cart_pole': 5.8e-14, 'random_17_3': 1.9e-15, 'random_32_32': 2.6e-14}


def bound(name):
    return max(rr.FACTOR * E_REF_TRAJ[name], rr.FLOOR)


def adj_bound(name):
    return max(rr.FACTOR * E_REF_TRAJ_ADJ[name], rr.FLOOR)
