"""The MPC step as a differentiable torch operation: ``u = mpc_step(controller, x, u_prev, xref)``.

Forward is ``BatchMPCController.step`` on device tensors (one library call: update + warm-started solve + output); backward is ONE
``mpcqp_adjoint`` call (include/mpcqp_adjoint.h) with ``g_u0 = grad_output``: the active-set KKT system of every instance is factored
once on the device and solved for the incoming gradient, and the chain rule into x, u_prev and xref happens in the same kernel.  torch
is the container of the device buffers and the owner of the graph; no torch operation computes anything of the solve or its derivative.

* Instances whose solve does not end 'solved' return ``u_failure`` (mpc.py:301-304), a constant: their gradient is zero.
* The gradient is that of the active set the iterate implies.  Solve tightly (eps 1e-6 or below) or with ``polish=True`` where it must
  be the true one; ``controller.prob.adjoint_info()`` after a backward tells how many rows were weakly active (a kink of the piecewise
  affine law: the gradient is one-sided there).
* The adjoint differentiates the solution the controller holds NOW.  A controller that has been stepped again between a forward and
  its backward holds another solution, so the backward raises; a rollout of several steps needs one controller per step (see
  examples/differentiable_mpc.py).  The library refuses on its own account where the controller's step data, model or iterate were replaced
  without a solve (``update(..., solve=False)``, ``update_model(solve=False)``, ``warm_start``): mpcqp_adjoint answers MPCQP_ERR_STATE
  until the next solve.
"""
import torch


def _sync_needed(K):
    """The library works on the controller's stream: unless that IS torch's current stream, the two are ordered by waiting."""
    return K.stream is None or int(K.stream) != int(torch.cuda.current_stream().cuda_stream)


class _MPCStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, K, x, u_prev, xref):
        if not x.is_cuda:
            raise ValueError('mpc_step works on device tensors (x is on %s)' % x.device)
        sync = _sync_needed(K)
        if sync:
            torch.cuda.current_stream().synchronize()
        det = lambda t: None if t is None else t.detach().to(torch.float64).contiguous()
        u = torch.empty((K.B, K.nu), dtype=torch.float64, device=x.device)
        xr = det(xref)
        K.step(det(x), det(u_prev), None if xr is None else xr.reshape(K.B, -1), out=u)
        if sync:
            K.prob.synchronize()
        ctx.K, ctx.count = K, K.solve_count
        ctx.shapes = tuple(None if t is None else tuple(t.shape) for t in (x, u_prev, xref))
        return u

    @staticmethod
    def backward(ctx, grad_u):
        K = ctx.K
        if K.solve_count != ctx.count:
            raise RuntimeError('mpc_step: the controller has been stepped or solved again since this forward (%d solves then, %d now); '
                               'its solution is no longer the one to differentiate.  Use one controller per step of a rollout.'
                               % (ctx.count, K.solve_count))
        names = ('x0', 'uminus1', 'xref')
        want = [n for n, need, shp in zip(names, ctx.needs_input_grad[1:], ctx.shapes) if need and shp is not None]
        if not want:
            return None, None, None, None
        sync = _sync_needed(K)
        if sync:
            torch.cuda.current_stream().synchronize()
        res = K.prob.adjoint(g_u0=grad_u.to(torch.float64).contiguous(), want=want)
        if sync:
            K.prob.synchronize()
        grads = [res[n].reshape(shp) if n in res else None for n, shp in zip(names, ctx.shapes)]
        return (None,) + tuple(grads)


def mpc_step(controller, x, u_prev=None, xref=None):
    """``u [B,nu] = K(x [B,nx], u_prev [B,nu], xref [B,nx] or [B,Np+1,nx])`` of a set-up ``BatchMPCController``, differentiable with
    respect to the three tensors (float64 device tensors; ``u_prev`` / ``xref`` None: the controller's own, no gradient)."""
    if controller.prob is None:
        raise RuntimeError('mpc_step needs a controller that has been set up')
    return _MPCStep.apply(controller, x, u_prev, xref)
