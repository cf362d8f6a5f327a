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
* ``params``: the model itself as an input of the layer -- a dict of device tensors under the names Ad, Bd, Qx, QxN, Qu, QDu, each
  [B, ...] (one per instance) or unbatched [...] (one model shared by the batch).  Forward puts them under the controller with
  ``update_model(solve=False, ...)`` (mpcqp_update_model: re-equilibrate, refactor, keep the iterate) and steps; backward asks ONE
  ``mpcqp_adjoint_model`` call (include/mpcqp_adjoint_model.h) for exactly the gradients torch needs, an unbatched parameter's as the sum
  over the batch formed on the device (``batch_sum``).  The weight gradients are those of a symmetric perturbation: a weight that is
  parametrized symmetric (Q = L L', a diagonal) gets its true gradient.
"""
import torch


def _sync_needed(K):
    """The library works on the controller's stream: unless that IS torch's current stream, the two are ordered by waiting."""
    return K.stream is None or int(K.stream) != int(torch.cuda.current_stream().cuda_stream)


MODEL_PARAMS = ('Ad', 'Bd', 'Qx', 'QxN', 'Qu', 'QDu')


class _MPCStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, K, x, u_prev, xref, names, *params):
        if not x.is_cuda:
            raise ValueError('mpc_step works on device tensors (x is on %s)' % x.device)
        sync = _sync_needed(K)
        if sync:
            torch.cuda.current_stream().synchronize()
        det = lambda t: None if t is None else t.detach().to(torch.float64).contiguous()
        if names:
            K.update_model(solve=False, **{n: det(p) for n, p in zip(names, params)})
        u = torch.empty((K.B, K.nu), dtype=torch.float64, device=x.device)
        xr = det(xref)
        K.step(det(x), det(u_prev), None if xr is None else xr.reshape(K.B, -1), out=u)
        if sync:
            K.prob.synchronize()
        ctx.K, ctx.count = K, K.solve_count
        ctx.shapes = tuple(None if t is None else tuple(t.shape) for t in (x, u_prev, xref))
        ctx.names, ctx.pshapes = names, tuple(tuple(p.shape) for p in params)
        return u

    @staticmethod
    def backward(ctx, grad_u):
        K = ctx.K
        if K.solve_count != ctx.count:
            raise RuntimeError('mpc_step: the controller has been stepped or solved again since this forward (%d solves then, %d now); '
                               'its solution is no longer the one to differentiate.  Use one controller per step of a rollout.'
                               % (ctx.count, K.solve_count))
        names = ('x0', 'uminus1', 'xref')
        want = [n for n, need, shp in zip(names, ctx.needs_input_grad[1:4], ctx.shapes) if need and shp is not None]
        pneed = [n for n, need in zip(ctx.names, ctx.needs_input_grad[5:]) if need]
        none = (None,) * (5 + len(ctx.names))
        if not want and not pneed:
            return none
        # one model for the whole batch: the device adds the instances' gradients up (a mixture of shared and per-instance parameters
        # takes them per instance and adds the shared ones' here)
        shared = {n: len(shp) == 2 for n, shp in zip(ctx.names, ctx.pshapes)}
        batch_sum = bool(pneed) and all(shared[n] for n in pneed)
        sync = _sync_needed(K)
        if sync:
            torch.cuda.current_stream().synchronize()
        res = K.prob.adjoint(g_u0=grad_u.to(torch.float64).contiguous(), want=want + pneed, batch_sum=batch_sum)
        if sync:
            K.prob.synchronize()
        grads = [res[n].reshape(shp) if n in res else None for n, shp in zip(names, ctx.shapes)]
        pgrads = []
        for n, shp in zip(ctx.names, ctx.pshapes):
            g = res.get(n)
            if g is not None:
                g = (g[0] if batch_sum else g.sum(dim=0)) if shared[n] else g
                g = g.reshape(shp)
            pgrads.append(g)
        return (None,) + tuple(grads) + (None,) + tuple(pgrads)


def mpc_step(controller, x, u_prev=None, xref=None, params=None):
    """``u [B,nu] = K(x [B,nx], u_prev [B,nu], xref [B,nx] or [B,Np+1,nx])`` of a set-up ``BatchMPCController``, differentiable with
    respect to the three tensors (float64 device tensors; ``u_prev`` / ``xref`` None: the controller's own, no gradient) and, with
    ``params`` -- a dict of device tensors under any of the names Ad, Bd, Qx, QxN, Qu, QDu, each [B, ...] or unbatched [...] -- with respect
    to the model the step is made with: the controller's model is replaced by them first (``update_model``)."""
    if controller.prob is None:
        raise RuntimeError('mpc_step needs a controller that has been set up')
    names = tuple(params) if params else ()
    for n in names:
        if n not in MODEL_PARAMS:
            raise TypeError('mpc_step: unknown model parameter %r (one of %s)' % (n, ', '.join(MODEL_PARAMS)))
        if not hasattr(params[n], 'data_ptr') or not params[n].is_cuda or params[n].dim() not in (2, 3):
            raise ValueError('mpc_step: params[%r] must be a device tensor [B, ., .] or [., .]' % n)
    return _MPCStep.apply(controller, x, u_prev, xref, names, *[params[n] for n in names])


# ---- a closed-loop rollout as one differentiable operation (include/mpcqp_rollout.h) ---------------------------------------------------
class _MPCRollout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, K, nsteps, x0, u_prev, xref, w, Ap, Bp, names, *params):
        if not x0.is_cuda:
            raise ValueError('mpc_rollout works on device tensors (x0 is on %s)' % x0.device)
        sync = _sync_needed(K)
        if sync:
            torch.cuda.current_stream().synchronize()
        det = lambda t: None if t is None else t.detach().to(torch.float64).contiguous()
        if names:
            K.update_model(solve=False, **{n: det(p) for n, p in zip(names, params)})
        xr = det(xref)
        K.update(det(x0), det(u_prev), None if xr is None else xr.reshape(K.B, -1))      # (and the solve for x_0: tape entry 0)
        kw = dict(dtype=torch.float64, device=x0.device)
        X, U = torch.empty((nsteps + 1, K.B, K.nx), **kw), torch.empty((nsteps, K.B, K.nu), **kw)
        st, it = (torch.empty((nsteps, K.B), dtype=torch.int32, device=x0.device) for _ in range(2))
        bc = lambda t, shape: None if t is None else det(t).expand(shape).contiguous()
        K.prob.rollout(nsteps, w=det(w), Ap=bc(Ap, (K.B, K.nx, K.nx)), Bp=bc(Bp, (K.B, K.nx, K.nu)), out=[X, U, st, it])
        K.solve_count += nsteps
        K.x0_rh, K.uminus1_rh, K._um1_on_device, K._u_last = X[-1], U[-1], True, None
        if sync:
            K.prob.synchronize()
        ctx.K, ctx.count = K, K.prob.rollout_count
        ctx.shapes = tuple(None if t is None else tuple(t.shape) for t in (x0, u_prev, xref, w, Ap, Bp))
        ctx.names, ctx.pshapes = names, tuple(tuple(p.shape) for p in params)
        ctx.status, ctx.iters = st, it
        return X, U

    @staticmethod
    def backward(ctx, grad_X, grad_U):
        K = ctx.K
        if K.prob.rollout_count != ctx.count:
            raise RuntimeError('mpc_rollout: the controller has been rolled out again since this forward (rollout %d then, %d now); '
                               'its tape is no longer the one to differentiate.' % (ctx.count, K.prob.rollout_count))
        need = dict(zip(('x0', 'u_prev', 'xref', 'w', 'Ap', 'Bp'), ctx.needs_input_grad[2:8]))
        need = {n: v and shp is not None for (n, v), shp in zip(need.items(), ctx.shapes)}
        pneed = [n for n, v in zip(ctx.names, ctx.needs_input_grad[9:]) if v]
        if not any(need.values()) and not pneed:
            return (None,) * (9 + len(ctx.names))
        own_plant = ctx.shapes[4] is not None
        # the controller's own model as the plant: Ad, Bd are then one parameter with two paths, and the plant's comes back on its own
        plant = [n for n, m in (('Ap', 'Ad'), ('Bp', 'Bd')) if (need[n] if own_plant else m in pneed)]
        want = ([n for n, k in (('lam', 'x0'), ('uminus1', 'u_prev'), ('xref', 'xref')) if need[k]] + (['lam'] if need['w'] and not need['x0'] else [])
                + plant + pneed)
        shared = {n: len(shp) == 2 for n, shp in zip(ctx.names, ctx.pshapes)}
        batch_sum = bool(pneed) and all(shared[n] for n in pneed)
        sync = _sync_needed(K)
        if sync:
            torch.cuda.current_stream().synchronize()
        res = K.prob.rollout_adjoint(g_x=grad_X.to(torch.float64).contiguous(), g_u=grad_U.to(torch.float64).contiguous(), want=want, batch_sum=batch_sum)
        if sync:
            K.prob.synchronize()
        g = lambda v, shp: None if v is None else v.reshape(shp)
        grads = [g(res['lam'][0] if need['x0'] else None, ctx.shapes[0]), g(res.get('uminus1'), ctx.shapes[1]),
                 g(res['xref'].sum(dim=0) if need['xref'] else None, ctx.shapes[2]), g(res['lam'][1:] if need['w'] else None, ctx.shapes[3])]
        for n, shp in (('Ap', ctx.shapes[4]), ('Bp', ctx.shapes[5])):
            v = res.get(n) if own_plant and need[n] else None
            grads.append(None if v is None else (v.sum(dim=0) if len(shp) == 2 else v).reshape(shp))
        pgrads = []
        for n, shp in zip(ctx.names, ctx.pshapes):
            v = res.get(n) if n in pneed else None
            if v is not None:
                v = (v[0] if batch_sum else v.sum(dim=0)) if shared[n] else v
                if not own_plant and n in ('Ad', 'Bd'):
                    p = res['Ap' if n == 'Ad' else 'Bp']
                    v = v + (p.sum(dim=0) if shared[n] else p)
                v = v.reshape(shp)
            pgrads.append(v)
        return (None, None) + tuple(grads) + (None,) + tuple(pgrads)


def mpc_rollout(controller, x0, nsteps, u_prev=None, xref=None, w=None, Ap=None, Bp=None, params=None):
    """``(X [K+1,B,nx], U [K,B,nu])`` of ``nsteps`` = K closed-loop steps of a set-up ``BatchMPCController`` from ``x0`` [B,nx] against the
    plant x_{k+1} = Ap x_k + Bp u_k + w[k] (``Ap`` / ``Bp`` None: the controller's own Ad, Bd; ``w`` [K,B,nx] or None), on ONE controller:
    forward is ``update_model(solve=False, **params)`` where given, ``update(x0, u_prev, xref)`` with its solve, then
    ``BatchMPCController.rollout``'s device loop with a tape (mpcqp_rollout); backward is ONE ``mpcqp_rollout_adjoint`` call with
    ``G_x = grad_X``, ``G_u = grad_U`` -- one reverse sweep over the tape on the device, which factors the active-set system of a step only
    where its active set differs from the step's behind it.  Differentiable with respect to ``x0``, ``u_prev``, ``xref`` (constant over
    the rollout), ``w``, ``Ap``, ``Bp`` ([B, ., .] or unbatched) and ``params`` (as in ``mpc_step``; with ``Ap`` / ``Bp`` None the gradients
    of ``params['Ad']`` / ``['Bd']`` include the plant path).  A step whose solve does not end 'solved' applies ``u_failure`` = uref and
    passes the gradient through the plant alone.  The tape is a copy: stepping or solving the controller between forward and backward is
    fine, another rollout is not -- the backward then raises."""
    if controller.prob is None:
        raise RuntimeError('mpc_rollout needs a controller that has been set up')
    names = tuple(params) if params else ()
    for n in names:
        if n not in MODEL_PARAMS:
            raise TypeError('mpc_rollout: unknown model parameter %r (one of %s)' % (n, ', '.join(MODEL_PARAMS)))
        if not hasattr(params[n], 'data_ptr') or not params[n].is_cuda or params[n].dim() not in (2, 3):
            raise ValueError('mpc_rollout: params[%r] must be a device tensor [B, ., .] or [., .]' % n)
    if (Ap is None) != (Bp is None):
        raise ValueError('mpc_rollout: give both Ap and Bp or neither')
    return _MPCRollout.apply(controller, int(nsteps), x0, u_prev, xref, w, Ap, Bp, names, *[params[n] for n in names])


# ---- the output-feedback rollout, differentiated through the estimator (include/mpcqp_rollout_est.h) -----------------------------------
class _MPCRolloutEst(torch.autograd.Function):
    @staticmethod
    def forward(ctx, K, nsteps, x0, xhat0, C, L, v, u_prev, xref, w, Ap, Bp, names, *params):
        if not x0.is_cuda:
            raise ValueError('mpc_rollout_est works on device tensors (x0 is on %s)' % x0.device)
        sync = _sync_needed(K)
        if sync:
            torch.cuda.current_stream().synchronize()
        det = lambda t: None if t is None else t.detach().to(torch.float64).contiguous()
        if names:
            K.update_model(solve=False, **{n: det(p) for n, p in zip(names, params)})
        xr = det(xref)
        K.update(det(xhat0), det(u_prev), None if xr is None else xr.reshape(K.B, -1))      # (and the solve for xhat_0: tape entry 0)
        ny = int(C.shape[-2])
        kw = dict(dtype=torch.float64, device=x0.device)
        X, XH, U = torch.empty((nsteps + 1, K.B, K.nx), **kw), torch.empty((nsteps + 1, K.B, K.nx), **kw), torch.empty((nsteps, K.B, K.nu), **kw)
        Y = torch.empty((nsteps, K.B, ny), **kw)
        st, it = (torch.empty((nsteps, K.B), dtype=torch.int32, device=x0.device) for _ in range(2))
        bc = lambda t, shape: None if t is None else det(t).expand(shape).contiguous()
        est = dict(C=bc(C, (K.B, ny, K.nx)), L=bc(L, (K.B, K.nx, ny)), x_true=det(x0).clone(), v=det(v))
        K.prob.rollout_est(nsteps, est, w=det(w), Ap=bc(Ap, (K.B, K.nx, K.nx)), Bp=bc(Bp, (K.B, K.nx, K.nu)), out=[X, U, st, it, XH, Y])
        K.solve_count += nsteps
        K.x0_rh, K.uminus1_rh, K._um1_on_device, K._u_last = XH[-1], U[-1], True, None
        if sync:
            K.prob.synchronize()
        ctx.K, ctx.count = K, K.prob.rollout_count
        ctx.shapes = tuple(None if t is None else tuple(t.shape) for t in (x0, xhat0, C, L, v, u_prev, xref, w, Ap, Bp))
        ctx.names, ctx.pshapes = names, tuple(tuple(p.shape) for p in params)
        ctx.status, ctx.iters = st, it
        return X, XH, Y, U

    @staticmethod
    def backward(ctx, grad_X, grad_XH, grad_Y, grad_U):
        K = ctx.K
        if K.prob.rollout_count != ctx.count:
            raise RuntimeError('mpc_rollout_est: the controller has been rolled out again since this forward (rollout %d then, %d now); '
                               'its tape is no longer the one to differentiate.' % (ctx.count, K.prob.rollout_count))
        inputs = ('x0', 'xhat0', 'C', 'L', 'v', 'u_prev', 'xref', 'w', 'Ap', 'Bp')
        need = {n: bool(v) and shp is not None for n, v, shp in zip(inputs, ctx.needs_input_grad[2:12], ctx.shapes)}
        shape = dict(zip(inputs, ctx.shapes))
        pneed = [n for n, v in zip(ctx.names, ctx.needs_input_grad[13:]) if v]
        none = (None,) * (13 + len(ctx.names))
        if not any(need.values()) and not pneed:
            return none
        own_plant = shape['Ap'] is not None
        # Ad, Bd are the estimator's model too, and without Ap, Bp the plant's: one parameter with three paths, two of which come back on their own
        plant = [n for n, m in (('Ap', 'Ad'), ('Bp', 'Bd')) if (need[n] if own_plant else m in pneed)]
        estp = [n for n, m in (('Ae', 'Ad'), ('Be', 'Bd')) if m in pneed]
        want = []
        if need['x0'] or need['w']:
            want.append('lam')
        want += [r for r, n in (('eta', 'xhat0'), ('C', 'C'), ('L', 'L'), ('v', 'v'), ('uminus1', 'u_prev'), ('xref', 'xref')) if need[n]]
        want += plant + estp + pneed
        shared = {n: len(shp) == 2 for n, shp in zip(ctx.names, ctx.pshapes)}
        batch_sum = bool(pneed) and all(shared[n] for n in pneed)
        sync = _sync_needed(K)
        if sync:
            torch.cuda.current_stream().synchronize()
        c64 = lambda t: t.to(torch.float64).contiguous()
        res = K.prob.rollout_adjoint(g_x=c64(grad_X), g_u=c64(grad_U), g_xhat=c64(grad_XH), g_y=c64(grad_Y), want=want, batch_sum=batch_sum)
        if sync:
            K.prob.synchronize()
        per = lambda v, shp, nd: None if v is None else (v.sum(dim=0) if len(shp) == nd - 1 else v).reshape(shp)      # (an unbatched input: summed over the batch)
        grads = [res['lam'][0].reshape(shape['x0']) if need['x0'] else None,
                 res['eta'][0].reshape(shape['xhat0']) if need['xhat0'] else None,
                 per(res.get('C') if need['C'] else None, shape['C'], 3), per(res.get('L') if need['L'] else None, shape['L'], 3),
                 res['v'].reshape(shape['v']) if need['v'] else None,
                 res['uminus1'].reshape(shape['u_prev']) if need['u_prev'] else None,
                 res['xref'].sum(dim=0).reshape(shape['xref']) if need['xref'] else None,
                 res['lam'][1:].reshape(shape['w']) if need['w'] else None,
                 per(res.get('Ap') if own_plant and need['Ap'] else None, shape['Ap'], 3),
                 per(res.get('Bp') if own_plant and need['Bp'] else None, shape['Bp'], 3)]
        pgrads = []
        for n, shp in zip(ctx.names, ctx.pshapes):
            v = res.get(n) if n in pneed else None
            if v is not None:
                v = (v[0] if batch_sum else v.sum(dim=0)) if shared[n] else v
                if n in ('Ad', 'Bd'):
                    for path in (('Ae', 'Be'),) + ((('Ap', 'Bp'),) if not own_plant else ()):
                        p = res[path[0] if n == 'Ad' else path[1]]
                        v = v + (p.sum(dim=0) if shared[n] else p)
                v = v.reshape(shp)
            pgrads.append(v)
        return (None, None) + tuple(grads) + (None,) + tuple(pgrads)


def mpc_rollout_est(controller, x0, xhat0, nsteps, C, L, v=None, u_prev=None, xref=None, w=None, Ap=None, Bp=None, params=None):
    """``(X [K+1,B,nx], Xhat [K+1,B,nx], Y [K,B,ny], U [K,B,nu])`` of ``nsteps`` = K steps of the OUTPUT-FEEDBACK loop of a set-up
    ``BatchMPCController``: the plant x_{k+1} = Ap x_k + Bp u_k + w[k] starts at ``x0`` [B,nx], the controller sees the estimate only, which
    starts at ``xhat0`` [B,nx] and follows xhat_{k+1} = Ad (xhat_k + L (y_k - C xhat_k)) + Bd u_k with y_k = C x_k + v[k] (``C`` [B,ny,nx] or
    [ny,nx], ``L`` [B,nx,ny] or [nx,ny], ``v`` [K,B,ny] or None).  Forward is ``update_model(solve=False, **params)`` where given,
    ``update(xhat0, u_prev, xref)`` with its solve, then the device loop with a tape (mpcqp_rollout_est); backward is ONE
    ``mpcqp_rollout_adjoint_est`` call with the four seeds ``grad_X, grad_Xhat, grad_Y, grad_U``.  Differentiable with respect to ``x0``,
    ``xhat0``, ``C``, ``L``, ``v``, ``u_prev``, ``xref``, ``w``, ``Ap``, ``Bp`` and ``params`` (as in ``mpc_rollout``); the gradients of
    ``params['Ad']`` / ``['Bd']`` include the estimator's path and, with ``Ap`` / ``Bp`` None, the plant's.  ``mpc_rollout`` is the loop
    without an estimator."""
    if controller.prob is None:
        raise RuntimeError('mpc_rollout_est needs a controller that has been set up')
    names = tuple(params) if params else ()
    for n in names:
        if n not in MODEL_PARAMS:
            raise TypeError('mpc_rollout_est: unknown model parameter %r (one of %s)' % (n, ', '.join(MODEL_PARAMS)))
        if not hasattr(params[n], 'data_ptr') or not params[n].is_cuda or params[n].dim() not in (2, 3):
            raise ValueError('mpc_rollout_est: params[%r] must be a device tensor [B, ., .] or [., .]' % n)
    if (Ap is None) != (Bp is None):
        raise ValueError('mpc_rollout_est: give both Ap and Bp or neither')
    for n, t in (('C', C), ('L', L)):
        if not hasattr(t, 'data_ptr') or not t.is_cuda or t.dim() not in (2, 3):
            raise ValueError('mpc_rollout_est: %s must be a device tensor [B, ., .] or [., .]' % n)
    return _MPCRolloutEst.apply(controller, int(nsteps), x0, xhat0, C, L, v, u_prev, xref, w, Ap, Bp, names, *[params[n] for n in names])
