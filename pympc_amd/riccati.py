"""Batched discrete algebraic Riccati equations on the device (include/mpcqp_riccati.h): ``dare`` and ``dare_adjoint`` are the two library
calls on numpy arrays or device tensors, ``kalman_gain`` and ``lqr_terminal`` the two designs made of them.  Their stepwise companions
(include_ext3/mpcqp_riccati_traj.h) are ``dre`` and ``dre_adjoint`` -- the Riccati difference equation over a model trajectory -- with
``kalman_gain_traj`` (the Kalman filter of a time-varying system) and ``lqr_traj`` (the cost-to-go of a model schedule) made of them.

    X = A'XA - A'XB (R + B'XB)^-1 B'XA + Q

Every matrix is [B, ., .] or unbatched [., .] (one for the whole batch); the results are unbatched only if every input is.  numpy in, numpy
out: the call copies through one staging block and waits.  Device tensors in, device tensors out on the same device: the call is ordered on
torch's current stream (or ``stream``) and returns without waiting.  ``status`` per instance: 1 converged, 0 not converged within
``max_iter`` (not stabilizable / detectable, overflow), -1 R or R + B'XB not positive definite; X, the gain and ``res`` of an instance that
did not converge are zeros.  Nothing here runs on the host but the bookkeeping: pympc_amd.kalman keeps the scipy designs.
"""
import ctypes as C

import numpy as np

from . import _lib

_NEEDS = 'the loaded library has no Riccati solver (include/mpcqp_riccati.h: mpcqp_dare, mpcqp_dare_adjoint); the CPU twin does not export it'


def _library():
    L = _lib.load()
    if not _lib.has_riccati(L):
        raise NotImplementedError(_NEEDS)
    return L


def _settings(gain_form, max_iter, tol):
    s = _lib.RiccatiSettings()
    _lib.load().mpcqp_riccati_default_settings(C.byref(s))
    if gain_form not in (0, 1):
        raise ValueError('gain_form must be 0 (K = M^-1 B\'XA) or 1 (F = M^-1 B\'X)')
    s.gain_form = int(gain_form)
    if max_iter is not None:
        s.max_iter = int(max_iter)
    if tol is not None:
        s.tol = float(tol)
    return s


class _Call:
    """The arrays of one call: all numpy or all tensors of one device, float64, C-contiguous, broadcast to the batch."""

    def __init__(self, fn, arrs, stream):
        given = [a for a in arrs.values() if a is not None]
        self.fn = fn
        self.torch = any(hasattr(a, 'data_ptr') for a in given)
        if self.torch:
            import torch
            if not all(hasattr(a, 'data_ptr') and a.is_cuda for a in given):
                raise ValueError('%s takes numpy arrays or device tensors, not a mixture and no host tensors' % fn)
            self.device = given[0].device
            if any(a.device != self.device for a in given):
                raise ValueError('%s: every tensor must be on the same device' % fn)
            self.index = self.device.index if self.device.index is not None else torch.cuda.current_device()
            self.stream = int(stream) if stream is not None else int(torch.cuda.current_stream(self.device).cuda_stream)
        else:
            self.index, self.stream = 0, (int(stream) if stream is not None else 0)
        dims = {k: (a.dim() if hasattr(a, 'dim') else np.ndim(a)) for k, a in arrs.items() if a is not None}
        for k, d in dims.items():
            if d not in (2, 3):
                raise ValueError('%s: %s must be [B, ., .] or [., .]' % (fn, k))
        sizes = {int(arrs[k].shape[0]) for k, d in dims.items() if d == 3}
        if len(sizes) > 1:
            raise ValueError('%s: the batched inputs disagree about the batch size: %s' % (fn, sorted(sizes)))
        self.batched = bool(sizes)
        self.B = sizes.pop() if sizes else 1

    def prep(self, a, shape, name):
        """[B] + shape, float64, contiguous (None stays None)."""
        if a is None:
            return None
        full = (self.B,) + tuple(shape)
        if tuple(a.shape[-len(shape):]) != tuple(shape):
            raise ValueError('%s: %s has shape %s, expected [B, %s] or [%s]' % (self.fn, name, tuple(a.shape), *(2 * (', '.join(map(str, shape)),))))
        if self.torch:
            import torch
            return a.detach().to(torch.float64).expand(full).contiguous()
        return np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), full))

    def new(self, shape, dtype=np.float64):
        if self.torch:
            import torch
            return torch.empty((self.B,) + tuple(shape), dtype=torch.float64 if dtype is np.float64 else torch.int32, device=self.device)
        return np.empty((self.B,) + tuple(shape), dtype=dtype)

    def ret(self, a):
        return a if self.batched or a is None else a[0]


def _arr(a):
    return a if a is None or hasattr(a, 'data_ptr') else np.asarray(a, dtype=np.float64)


def _ptr(a):
    if a is None:
        return None
    return C.c_void_p(a.data_ptr() if hasattr(a, 'data_ptr') else a.ctypes.data)


def _fold(A, B, Q, R, S):
    """The equation with a cross term S [n, m] as one without: A - B R^-1 S', Q - S R^-1 S' (and what the gain of form 0 gets back: R^-1 S')."""
    if hasattr(R, 'data_ptr'):
        import torch
        RiSt = torch.linalg.solve(R, S.transpose(-1, -2))
    else:
        A, B, Q, R, S = (np.asarray(M, dtype=float) for M in (A, B, Q, R, S))
        RiSt = np.linalg.solve(R, np.swapaxes(S, -1, -2))
    return A - B @ RiSt, Q - S @ RiSt, RiSt


def dare(A, B, Q, R, S=None, gain_form=0, max_iter=None, tol=None, stream=None):
    """``X, K, status, iters, res`` of mpcqp_dare: the solution, the gain -- ``gain_form`` 0: K = (R + B'XB)^-1 B'XA (LQR / predictor form),
    1: F = (R + B'XB)^-1 B'X (filter form), both [m, n] --, the outcome, the doubling steps taken and the relative residual per instance.
    ``S`` [n, m]: a cross term x'Su of the cost, folded in before the call (gain_form 0 only; the gain returned is the whole one,
    (R + B'XB)^-1 (B'XA + S'))."""
    L = _library()
    A, B, Q, R, S = (_arr(M) for M in (A, B, Q, R, S))
    back = None
    if S is not None:
        if gain_form != 0:
            raise ValueError('dare: a cross term S goes with gain_form 0 only')
        A, Q, back = _fold(A, B, Q, R, S)
    c = _Call('dare', dict(A=A, B=B, Q=Q, R=R), stream)
    n, m = int(B.shape[-2]), int(B.shape[-1])
    A, B, Q, R = c.prep(A, (n, n), 'A'), c.prep(B, (n, m), 'B'), c.prep(Q, (n, n), 'Q'), c.prep(R, (m, m), 'R')
    X, K, status, iters, res = c.new((n, n)), c.new((m, n)), c.new((), np.int32), c.new((), np.int32), c.new(())
    s = _settings(gain_form, max_iter, tol)
    _lib.check(L.mpcqp_dare(c.index, c.stream, c.B, n, m, C.byref(s), _ptr(A), _ptr(B), _ptr(Q), _ptr(R),
                            _ptr(X), _ptr(K), _ptr(status), _ptr(iters), _ptr(res)), 'mpcqp_dare')
    if back is not None:
        ok = (status == 1).reshape(c.B, 1, 1)
        K = K + ok * back                                  # (an instance that did not converge keeps its zeros)
    return c.ret(X), c.ret(K), c.ret(status), c.ret(iters), c.ret(res)


def dare_adjoint(A, B, Q, R, X, K, status=None, G_X=None, G_K=None, gain_form=0, max_iter=None, tol=None, want=('A', 'B', 'Q', 'R'), stream=None):
    """The gradients of <G_X, X> + <G_K, K> with respect to A, B, Q, R at the solution ``X, K, status`` that ``dare`` returned under the same
    ``gain_form`` (mpcqp_dare_adjoint; no cross term): a dict by the names in ``want``, plus 'iters' (the steps of its Lyapunov iteration).
    The gradients of Q and R are those of a symmetric perturbation and are exactly symmetric; an instance whose status is not 1 gets zeros."""
    L = _library()
    if G_X is None and G_K is None:
        raise ValueError('dare_adjoint: give a seed, G_X or G_K')
    A, B, Q, R, X, K, G_X, G_K = (_arr(M) for M in (A, B, Q, R, X, K, G_X, G_K))
    want = tuple(want)
    if not want or any(w not in ('A', 'B', 'Q', 'R') for w in want):
        raise ValueError("dare_adjoint: want must name some of 'A', 'B', 'Q', 'R'")
    c = _Call('dare_adjoint', dict(A=A, B=B, Q=Q, R=R, X=X, K=K, G_X=G_X, G_K=G_K), stream)
    n, m = int(B.shape[-2]), int(B.shape[-1])
    shapes = dict(A=(n, n), B=(n, m), Q=(n, n), R=(m, m))
    A, B, Q, R = (c.prep(M, shapes[k], k) for k, M in zip('ABQR', (A, B, Q, R)))
    X, K, G_X, G_K = c.prep(X, (n, n), 'X'), c.prep(K, (m, n), 'K'), c.prep(G_X, (n, n), 'G_X'), c.prep(G_K, (m, n), 'G_K')
    if status is not None:
        if c.torch:
            import torch
            status = status.detach().to(torch.int32).reshape(-1).expand(c.B).contiguous()
        else:
            status = np.ascontiguousarray(np.broadcast_to(np.asarray(status, dtype=np.int32).reshape(-1), (c.B,)))
    out = {k: c.new(shapes[k]) for k in want}
    iters = c.new((), np.int32)
    s = _settings(gain_form, max_iter, tol)
    _lib.check(L.mpcqp_dare_adjoint(c.index, c.stream, c.B, n, m, C.byref(s), _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(X), _ptr(K),
                                    _ptr(status), _ptr(G_X), _ptr(G_K), *[_ptr(out.get(k)) for k in 'ABQR'], _ptr(iters)), 'mpcqp_dare_adjoint')
    res = {k: c.ret(v) for k, v in out.items()}
    res['iters'] = c.ret(iters)
    return res


def _t(M):
    """The transposed matrices as arrays of their own (the library reads plain row-major storage)."""
    return M.transpose(-1, -2).contiguous() if hasattr(M, 'data_ptr') else np.ascontiguousarray(np.swapaxes(np.asarray(M, dtype=float), -1, -2))


def kalman_gain(A, C, Qn, Rn, type='filter', **kw):
    """``L, P, status`` of the stationary Kalman filter / predictor of x+ = A x + w, y = C x + v, E[ww'] = Qn, E[vv'] = Rn: the dual problem
    (A', C', Qn, Rn) on the device, with the meaning of ``pympc_amd.kalman.kalman_design_simple`` -- 'filter': L = P C' (C P C' + Rn)^-1,
    'predictor': L = A P C' (C P C' + Rn)^-1 --; L is [nx, ny]."""
    if type not in ('filter', 'predictor'):
        raise ValueError("Unknown Kalman design type. Specify either filter or predictor!")
    P, G, status, _, _ = dare(_t(A), _t(C), Qn, Rn, gain_form=1 if type == 'filter' else 0, **kw)
    return _t(G), P, status


def lqr_terminal(Ad, Bd, Qx, Qu, **kw):
    """``X, K`` of the infinite-horizon LQR problem of (Ad, Bd, Qx, Qu): the cost-to-go x'Xx -- the terminal weight QxN that makes a finite
    horizon the infinite one while no constraint is active -- and the gain of u = -K x.  Raises if an instance did not converge."""
    X, K, status, _, _ = dare(Ad, Bd, Qx, Qu, **kw)
    bad = int((status != 1).sum())
    if bad:
        raise RuntimeError('lqr_terminal: %d instance(s) without a solution (status 0: not stabilizable / detectable, -1: Qu not positive definite)' % bad)
    return X, K


# ---- the Riccati difference equation (include_ext3/mpcqp_riccati_traj.h) ----------------------------------------------------------------
_NEEDS_TRAJ = ('the loaded library has no Riccati difference equation (include_ext3/mpcqp_riccati_traj.h: mpcqp_dre, mpcqp_dre_adjoint); '
               'the CPU twin does not export it')


def _traj_library():
    L = _lib.load()
    if not _lib.has_riccati_traj(L):
        raise NotImplementedError(_NEEDS_TRAJ)
    return L


def _ndim(a):
    return a.dim() if hasattr(a, 'dim') else np.ndim(a)


def traj_flags(fn, A, B, others):
    """``(A is a trajectory, B is a trajectory)`` by the number of dimensions: a call is batched if one of ``others`` (the per-instance
    matrices Q, R, X0) is [B, ., .] or A or B is [T, B, ., .]; [., ., .] is then one matrix per instance, and a trajectory [T, ., .] of
    unbatched matrices where nothing is batched."""
    for k, a in (('A', A), ('B', B)):
        if _ndim(a) not in (2, 3, 4):
            raise ValueError('%s: %s must be [n, .], [B, n, .], [T, n, .] or [T, B, n, .]' % (fn, k))
    batched = any(_ndim(a) == 3 for a in others if a is not None) or _ndim(A) == 4 or _ndim(B) == 4
    return tuple(_ndim(a) == 4 or (_ndim(a) == 3 and not batched) for a in (A, B))


class _TrajCall(_Call):
    """``_Call`` for a recursion: A and B with a flag each (a trajectory [T, B, ., .] / [T, ., .], or per-instance [B, ., .] / [., .]), the
    per-instance matrices ``consts`` and the arrays ``trajs`` that are trajectories by their meaning (X_traj, G_X, G_K)."""

    def __init__(self, fn, A, a_traj, B, b_traj, consts, trajs, T, stream):
        for k, a, tr in (('A', A, a_traj), ('B', B, b_traj)):
            if _ndim(a) not in ((3, 4) if tr else (2, 3)):
                raise ValueError('%s: %s must be %s' % (fn, k, '[T, B, ., .] or [T, ., .]' if tr else '[B, ., .] or [., .]'))
        for k, a in trajs.items():
            if a is not None and _ndim(a) not in (3, 4):
                raise ValueError('%s: %s must be [steps, B, ., .] or [steps, ., .]' % (fn, k))
        steps = {int(a.shape[0]) for a, tr in ((A, a_traj), (B, b_traj)) if tr}
        if len(steps) > 1:
            raise ValueError('%s: the trajectories of A and B disagree about the number of steps: %s' % (fn, sorted(steps)))
        if steps:
            if T is not None and int(T) != min(steps):
                raise ValueError('%s: T = %d, but the trajectories have %d entries' % (fn, int(T), min(steps)))
            T = min(steps)
        elif T is None:
            raise ValueError('%s: neither A nor B is a trajectory: give the number of steps T' % fn)
        self.T = int(T)
        if self.T < 1:
            raise ValueError('%s: T must be at least 1' % fn)
        rep = dict(consts, A=A[0] if a_traj else A, B=B[0] if b_traj else B)
        rep.update({k: (None if a is None else a[0]) for k, a in trajs.items()})
        super().__init__(fn, rep, stream)
        self.a_traj, self.b_traj = bool(a_traj), bool(b_traj)

    def prep_traj(self, a, steps, shape, name):
        """[steps, B] + shape, float64, contiguous (None stays None)."""
        if a is None:
            return None
        if int(a.shape[0]) != steps or tuple(a.shape[-len(shape):]) != tuple(shape):
            raise ValueError('%s: %s has shape %s, expected [%d, B, %s] or [%d, %s]' % (self.fn, name, tuple(a.shape), steps, ', '.join(map(str, shape)), steps, ', '.join(map(str, shape))))
        full = (steps, self.B) + tuple(shape)
        if self.torch:
            import torch
            a = a.detach().to(torch.float64)
            return (a if a.dim() == 4 else a.unsqueeze(1)).expand(full).contiguous()
        a = np.asarray(a, dtype=np.float64)
        return np.ascontiguousarray(np.broadcast_to(a if a.ndim == 4 else a[:, None], full))

    def model(self, a, tr, shape, name):
        return self.prep_traj(a, self.T, shape, name) if tr else self.prep(a, shape, name)

    def new_traj(self, steps, shape):
        if self.torch:
            import torch
            return torch.empty((steps, self.B) + tuple(shape), dtype=torch.float64, device=self.device)
        return np.empty((steps, self.B) + tuple(shape))

    def ret_traj(self, a):
        return a if self.batched or a is None else a[:, 0]


def _gain_form(fn, gain_form):
    if gain_form not in (0, 1):
        raise ValueError('%s: gain_form must be 0 (K = S^-1 B\'XA) or 1 (F = S^-1 B\'X)' % fn)
    s = _lib.RiccatiSettings()
    s.struct_size, s.max_iter, s.gain_form, s.tol = C.sizeof(_lib.RiccatiSettings), 1, int(gain_form), 0.0      # (max_iter and tol are ignored)
    return s


def dre_flagged(A, a_traj, B, b_traj, Q, R, X0, gain_form=0, T=None, stream=None):
    """``dre`` with the two trajectory flags given instead of read off the dimensions."""
    A, B, Q, R, X0 = (_arr(M) for M in (A, B, Q, R, X0))
    s = _gain_form('dre', gain_form)
    c = _TrajCall('dre', A, a_traj, B, b_traj, dict(Q=Q, R=R, X0=X0), {}, T, stream)
    n, m = int(B.shape[-2]), int(B.shape[-1])
    A, B = c.model(A, a_traj, (n, n), 'A'), c.model(B, b_traj, (n, m), 'B')
    Q, R, X0 = c.prep(Q, (n, n), 'Q'), c.prep(R, (m, m), 'R'), c.prep(X0, (n, n), 'X0')
    L = _traj_library()
    X, K, status, bad = c.new_traj(c.T + 1, (n, n)), c.new_traj(c.T, (m, n)), c.new((), np.int32), c.new((), np.int32)
    _lib.check(L.mpcqp_dre(c.index, c.stream, c.B, n, m, c.T, C.byref(s), _ptr(A), c.T if a_traj else 1, _ptr(B), c.T if b_traj else 1,
                           _ptr(Q), _ptr(R), _ptr(X0), _ptr(X), _ptr(K), _ptr(status), _ptr(bad)), 'mpcqp_dre')
    return c.ret_traj(X), c.ret_traj(K), c.ret(status), c.ret(bad)


def dre(A, B, Q, R, X0, gain_form=0, T=None, stream=None):
    """``X_traj [T+1, ..], K_traj [T, ..], status, first_bad`` of mpcqp_dre: from X_0 = sym(X0), for t = 0 .. T-1,

        S_t = R + B_t'X_t B_t,   gain_t = S_t^-1 B_t'X_t A_t (``gain_form`` 0) or S_t^-1 B_t'X_t (1),   X_{t+1} = sym(A_t'X_t A_t - A_t'X_t B_t K_t + Q).

    A and B are each one matrix ([B, n, .] or unbatched [n, .]) used at every step, or a trajectory with one more leading dimension
    ([T, B, n, .] / [T, n, .]); Q, R, X0 are [B, ., .] or [., .].  [., ., .] is read as [B, n, .] where the call is batched (Q, R or X0 is, or
    the other of A and B is [T, B, ., .]) and as a trajectory [T, n, .] where nothing is.  ``T``: the number of steps, needed where neither
    A nor B is a trajectory.  numpy or device tensors under the rules of ``dare``; the trajectories come back [steps, B, ., .], or
    [steps, ., .] if every input is unbatched.  ``status``: 1 done, -1 some S_t not positive definite, 0 a NaN or inf; ``first_bad``: the
    step at which the instance ended (-1: it ran through).  An instance that is not 1 gets zeros."""
    a_traj, b_traj = traj_flags('dre', _arr(A), _arr(B), [_arr(M) for M in (Q, R, X0)])
    return dre_flagged(A, a_traj, B, b_traj, Q, R, X0, gain_form=gain_form, T=T, stream=stream)


_TRAJ_WANT = ('A', 'B', 'Q', 'R', 'X0')


def dre_adjoint_flagged(A, a_traj, B, b_traj, Q, R, X0, X_traj, status=None, G_X=None, G_K=None, gain_form=0, T=None, want=_TRAJ_WANT, stream=None):
    """``dre_adjoint`` with the two trajectory flags given instead of read off the dimensions."""
    if G_X is None and G_K is None:
        raise ValueError('dre_adjoint: give a seed, G_X or G_K')
    want = tuple(want)
    if not want or any(w not in _TRAJ_WANT for w in want):
        raise ValueError("dre_adjoint: want must name some of 'A', 'B', 'Q', 'R', 'X0'")
    A, B, Q, R, X0, X_traj, G_X, G_K = (_arr(M) for M in (A, B, Q, R, X0, X_traj, G_X, G_K))
    s = _gain_form('dre_adjoint', gain_form)
    c = _TrajCall('dre_adjoint', A, a_traj, B, b_traj, dict(Q=Q, R=R, X0=X0), dict(X_traj=X_traj, G_X=G_X, G_K=G_K), T, stream)
    n, m = int(B.shape[-2]), int(B.shape[-1])
    A, B = c.model(A, a_traj, (n, n), 'A'), c.model(B, b_traj, (n, m), 'B')
    Q, R, X0 = c.prep(Q, (n, n), 'Q'), c.prep(R, (m, m), 'R'), c.prep(X0, (n, n), 'X0')
    X_traj, G_X, G_K = c.prep_traj(X_traj, c.T + 1, (n, n), 'X_traj'), c.prep_traj(G_X, c.T + 1, (n, n), 'G_X'), c.prep_traj(G_K, c.T, (m, n), 'G_K')
    if status is not None:
        if c.torch:
            import torch
            status = status.detach().to(torch.int32).reshape(-1).expand(c.B).contiguous()
        else:
            status = np.ascontiguousarray(np.broadcast_to(np.asarray(status, dtype=np.int32).reshape(-1), (c.B,)))
    L = _traj_library()
    out = {}
    for k in want:
        if (k == 'A' and a_traj) or (k == 'B' and b_traj):
            out[k] = c.new_traj(c.T, (n, n) if k == 'A' else (n, m))
        else:
            out[k] = c.new(dict(A=(n, n), B=(n, m), Q=(n, n), R=(m, m), X0=(n, n))[k])
    _lib.check(L.mpcqp_dre_adjoint(c.index, c.stream, c.B, n, m, c.T, C.byref(s), _ptr(A), c.T if a_traj else 1, _ptr(B), c.T if b_traj else 1,
                                   _ptr(Q), _ptr(R), _ptr(X0), _ptr(X_traj), _ptr(status), _ptr(G_X), _ptr(G_K),
                                   *[_ptr(out.get(k)) for k in _TRAJ_WANT]), 'mpcqp_dre_adjoint')
    return {k: (c.ret_traj(v) if (k == 'A' and a_traj) or (k == 'B' and b_traj) else c.ret(v)) for k, v in out.items()}


def dre_adjoint(A, B, Q, R, X0, X_traj, status=None, G_X=None, G_K=None, gain_form=0, T=None, want=_TRAJ_WANT, stream=None):
    """The gradients of sum_t <G_X[t], X_t> + sum_t <G_K[t], gain_t> (G_X [T+1, ..], G_K [T, ..]; either may be None) with respect to A, B,
    Q, R and X0 at the ``X_traj, status`` that ``dre`` returned for the same inputs under the same ``gain_form`` (mpcqp_dre_adjoint): a dict
    by the names in ``want``.  The gradient of a trajectory is one per entry, that of one matrix the sum over the steps; those of Q, R
    and X0 are gradients of a symmetric perturbation and exactly symmetric; an instance whose status is not 1 gets zeros."""
    a_traj, b_traj = traj_flags('dre_adjoint', _arr(A), _arr(B), [_arr(M) for M in (Q, R, X0)])
    return dre_adjoint_flagged(A, a_traj, B, b_traj, Q, R, X0, X_traj, status=status, G_X=G_X, G_K=G_K, gain_form=gain_form, T=T, want=want, stream=stream)


def _hold(hold):
    if int(hold) != hold or int(hold) < 1:
        raise ValueError('hold must be an integer >= 1')
    return int(hold)


def _repeat(a, hold):
    """Every entry of a trajectory ``hold`` times, by index."""
    if hold == 1:
        return a
    if hasattr(a, 'data_ptr'):
        import torch
        return a[torch.arange(a.shape[0], device=a.device).repeat_interleave(hold)]
    return a[np.repeat(np.arange(a.shape[0]), hold)]


def _flip(a):
    if hasattr(a, 'data_ptr'):
        import torch
        return torch.flip(a, [0])
    return np.ascontiguousarray(a[::-1])


def kalman_gain_traj(A_traj, C, Qn, Rn, P0, hold=1, stream=None):
    """``L_traj [nentries, B, nx, ny], P_traj [nentries + 1, B, nx, nx], status`` of the Kalman filter of the time-varying system
    x+ = A_e x + w, y = C x + v, E[ww'] = Qn, E[vv'] = Rn, in which entry e = k // hold of ``A_traj`` ([nentries, B, nx, nx] or
    [nentries, nx, nx]) is in force at step k and the estimate the filter starts from has covariance ``P0``: ``dre`` of the dual problem
    (A' -> A, C' -> B, gain_form 1, L = F').  With P_k the covariance of the estimate BEFORE the measurement of step k (P_0 = P0),

        L_k = P_k C' (C P_k C' + Rn)^-1,        P_{k+1} = A_e (P_k - L_k C P_k) A_e' + Qn,

    which is the order of the device loop (xhat_{k+1} = A_e (xhat_k + L (y_k - C xhat_k)) + B_e u_k: update, then predict): entry e of
    ``L_traj`` is L_k and entry e of ``P_traj`` is P_k at the entry's first step k = e hold, the last entry of ``P_traj`` is the covariance
    behind the last step.  ``run(estimator=, model_traj=(A_traj, None, hold), L_traj=L_traj)`` with hold = 1 is that filter."""
    hold = _hold(hold)
    A_traj = _arr(A_traj)
    if _ndim(A_traj) not in (3, 4):
        raise ValueError('kalman_gain_traj: A_traj must be [nentries, B, nx, nx] or [nentries, nx, nx]')
    return _dre_dual(dre_flagged, A_traj, C, Qn, Rn, P0, hold, stream)


def _dre_dual(call, A_traj, C, Qn, Rn, P0, hold, stream):
    X, F, status, _ = call(_repeat(_t(A_traj), hold), True, _t(_arr(C)), False, Qn, Rn, P0, gain_form=1, stream=stream)
    return _t(F[::hold]), X[::hold], status


def lqr_traj(Ad_traj, Bd_traj, Qx, Qu, QxN, stream=None):
    """``P_traj [T + 1, ..], K_traj [T, ..]`` of the finite-horizon LQR problem under the model schedule ``Ad_traj`` / ``Bd_traj`` (each
    [T, B, ., .] or [T, ., .]; step t runs under entry t) with terminal weight ``QxN``: ``P_traj[t]`` is the cost-to-go x'P x of the schedule
    from step t (``P_traj[T]`` = QxN, ``P_traj[0]`` the terminal weight that stands for the whole schedule) and ``K_traj[t]`` the gain of
    u_t = -K_t x_t.  The recursion of ``dre`` on the reversed schedule from X0 = QxN, returned in forward time order.  Raises if an
    instance did not run through."""
    Ad_traj, Bd_traj = _arr(Ad_traj), _arr(Bd_traj)
    for k, a in (('Ad_traj', Ad_traj), ('Bd_traj', Bd_traj)):
        if _ndim(a) not in (3, 4):
            raise ValueError('lqr_traj: %s must be [T, B, ., .] or [T, ., .]' % k)
    X, K, status, _ = dre_flagged(_flip(Ad_traj), True, _flip(Bd_traj), True, Qx, Qu, QxN, gain_form=0, stream=stream)
    bad = int((status != 1).sum())
    if bad:
        raise RuntimeError('lqr_traj: %d instance(s) did not run through (status -1: Qu + B\'PB not positive definite, 0: a NaN or inf)' % bad)
    return _flip(X), _flip(K)
