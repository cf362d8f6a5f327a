"""Batched discrete algebraic Riccati equations on the device (include/mpcqp_riccati.h): ``dare`` and ``dare_adjoint`` are the two library
calls on numpy arrays or device tensors, ``kalman_gain`` and ``lqr_terminal`` the two designs made of them.

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
