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
* ``bounds``: the constraint bounds as an input of the layer -- a dict of device tensors under the names xmin, xmax, umin, umax, Dumin,
  Dumax, each [B, nx | nu] or unbatched [nx | nu].  They go under the controller in the same ``update_model`` call as ``params``; backward
  asks the same one adjoint call (mpcqp_adjoint_bounds / mpcqp_rollout_adjoint_bounds, include/mpcqp_adjoint_bounds.h) for their
  gradients too: the multipliers of the active rows summed onto the bound each sits on, zero for a bound that is nowhere active.

A closed-loop rollout is one differentiable operation in five forms -- ``mpc_rollout`` (state feedback on one model), ``mpc_rollout_est``
(output feedback), ``mpc_rollout_tv`` (under a model schedule), ``mpc_rollout_tv_est`` (both), ``mpc_rollout_affine`` (state feedback with an
affine term in the prediction model, with or without a model schedule) -- which are one description: each Function
states its inputs and which options are present, ``_rollout_forward`` makes the taped loop of ``BatchProblem`` they pick, ``_rollout_backward``
asks ONE ``rollout_adjoint`` call for exactly the gradients torch needs, and ``_model_paths`` is the rule by which the gradient of a model
matrix is added up from its solve, estimator and plant paths.  The Riccati equations (``dare``, ``dre``) and the Kalman gains made of them
are differentiable operations of their own at the end of the file.
"""
import contextlib

import torch


MODEL_PARAMS = ('Ad', 'Bd', 'Qx', 'QxN', 'Qu', 'QDu')
BOUND_PARAMS = ('xmin', 'xmax', 'umin', 'umax', 'Dumin', 'Dumax')      # (the outputs of mpcqp_adjoint_bounds_io: pympc_amd._lib.ADJOINT_BOUNDS_NAMES)


# ---- what the step and the four rollouts share ------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _ordered(K):
    """The library works on the controller's stream: unless that IS torch's current stream, the two are ordered by waiting, torch's work
    before the library's and the library's before what torch does next."""
    sync = K.stream is None or int(K.stream) != int(torch.cuda.current_stream().cuda_stream)
    if sync:
        torch.cuda.current_stream().synchronize()
    yield
    if sync:
        K.prob.synchronize()


def _det(t):
    return None if t is None else t.detach().to(torch.float64).contiguous()


def _bc(t, shape):
    """A matrix given once for the batch or per instance, as the library takes it: per instance."""
    return None if t is None else _det(t).expand(shape).contiguous()


def _check_args(fn, controller, params, Ap=None, Bp=None, bounds=None):
    """What the public functions refuse; returns (the names of ``params`` in their order followed by those of ``bounds``, their tensors)."""
    if controller.prob is None:
        raise RuntimeError('%s needs a controller that has been set up' % fn)
    names = tuple(params) if params else ()
    for n in names:
        if n not in MODEL_PARAMS:
            raise TypeError('%s: unknown model parameter %r (one of %s)' % (fn, n, ', '.join(MODEL_PARAMS)))
        if not hasattr(params[n], 'data_ptr') or not params[n].is_cuda or params[n].dim() not in (2, 3):
            raise ValueError('%s: params[%r] must be a device tensor [B, ., .] or [., .]' % (fn, n))
    bnames = tuple(bounds) if bounds else ()
    for n in bnames:
        if n not in BOUND_PARAMS:
            raise TypeError('%s: unknown bound %r (one of %s)' % (fn, n, ', '.join(BOUND_PARAMS)))
        if not hasattr(bounds[n], 'data_ptr') or not bounds[n].is_cuda or bounds[n].dim() not in (1, 2):
            raise ValueError('%s: bounds[%r] must be a device tensor [B, .] or [.]' % (fn, n))
    if (Ap is None) != (Bp is None):
        raise ValueError('%s: give both Ap and Bp or neither' % fn)
    return names + bnames, [params[n] for n in names] + [bounds[n] for n in bnames]


def _put_params(ctx, K, names, params):
    """Forward: the parameters -- model and bounds, one ``update_model`` call -- go under the controller (no solve yet); their names and shapes
    are what backward assembles gradients by."""
    if names:
        K.update_model(solve=False, **{n: _det(p) for n, p in zip(names, params)})
    ctx.names, ctx.pshapes = names, tuple(tuple(p.shape) for p in params)


def _param_want(ctx, needs, also=()):
    """(the parameters, bounds among them, that need a gradient, which parameters are unbatched, batch_sum).  One model for the whole batch: the device adds the
    instances' gradients up (a mixture of shared and per-instance parameters takes them per instance and adds the shared ones' here).
    ``also``: is it unbatched, for every other input whose gradient ``batch_sum`` would sum -- under a schedule, whatever ``rollout_adjoint`` puts
    together from per-entry buffers."""
    pneed = [n for n, need in zip(ctx.names, needs) if need]
    shared = {n: len(shp) == (1 if n in BOUND_PARAMS else 2) for n, shp in zip(ctx.names, ctx.pshapes)}
    return pneed, shared, bool(pneed or also) and all(shared[n] for n in pneed) and all(also)


def _param_grads(ctx, res, pneed, shared, batch_sum, paths={}, sched=False):
    """The gradient of every parameter, None where none is needed.  ``paths``: parameter -> the gradients of ``res`` whose sum, in their order,
    is its own (Ad and Bd of a rollout: ``_model_paths``); any other parameter's is the one under its name.
    An unbatched parameter gets the sum over the batch, and which sweep returns what decides how it is read.  With ``batch_sum`` every adjoint
    call returns the model's and the bounds' gradients summed on the device, [1, ...]: ``p[0]``.  The plant's and the estimator's paths ('Ap',
    'Ae', ...) come summed only from the sweep under a schedule (``sched``), where ``BatchProblem.rollout_adjoint`` puts them together from
    per-entry buffers; the unscheduled sweep returns them per instance whatever ``batch_sum`` says: ``p.sum(dim=0)``."""
    pgrads = []
    for n, shp in zip(ctx.names, ctx.pshapes):
        v = None
        for g in paths.get(n, [n]) if n in pneed else ():
            p = res[g]
            if shared[n]:
                p = p[0] if batch_sum and (sched or g == n) else p.sum(dim=0)
            v = p.reshape(shp) if v is None else v + p.reshape(shp)
        pgrads.append(v)
    return pgrads


class _MPCStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, K, x, u_prev, xref, d, names, *params):
        if not x.is_cuda:
            raise ValueError('mpc_step works on device tensors (x is on %s)' % x.device)
        with _ordered(K):
            _put_params(ctx, K, names, params)
            u = torch.empty((K.B, K.nu), dtype=torch.float64, device=x.device)
            xr = _det(xref)
            dd = _det(d)
            K.step(_det(x), _det(u_prev), None if xr is None else xr.reshape(K.B, -1), out=u, d=None if dd is None else dd.reshape(K.B, -1))
        ctx.K, ctx.count = K, K.solve_count
        ctx.shapes = tuple(None if t is None else tuple(t.shape) for t in (x, u_prev, xref, d))
        return u

    @staticmethod
    def backward(ctx, grad_u):
        K = ctx.K
        if K.solve_count != ctx.count:
            raise RuntimeError('mpc_step: the controller has been stepped or solved again since this forward (%d solves then, %d now); '
                               'its solution is no longer the one to differentiate.  Use one controller per step of a rollout.'
                               % (ctx.count, K.solve_count))
        names = ('x0', 'uminus1', 'xref', 'd')      # ('d': the affine term the step was made with, mpcqp_adjoint_affine)
        want = [n for n, need, shp in zip(names, ctx.needs_input_grad[1:5], ctx.shapes) if need and shp is not None]
        pneed, shared, batch_sum = _param_want(ctx, ctx.needs_input_grad[6:])
        if not want and not pneed:
            return (None,) * (6 + len(ctx.names))
        with _ordered(K):
            res = K.prob.adjoint(g_u0=grad_u.to(torch.float64).contiguous(), want=want + pneed, batch_sum=batch_sum)
        grads = [res[n].reshape(shp) if n in res else None for n, shp in zip(names, ctx.shapes)]
        return (None,) + tuple(grads) + (None,) + tuple(_param_grads(ctx, res, pneed, shared, batch_sum))


def mpc_step(controller, x, u_prev=None, xref=None, params=None, bounds=None, d=None):
    """``u [B,nu] = K(x [B,nx], u_prev [B,nu], xref [B,nx] or [B,Np+1,nx])`` of a set-up ``BatchMPCController``, differentiable with
    respect to the three tensors (float64 device tensors; ``u_prev`` / ``xref`` None: the controller's own, no gradient) and, with
    ``params`` -- a dict of device tensors under any of the names Ad, Bd, Qx, QxN, Qu, QDu, each [B, ...] or unbatched [...] -- with respect
    to the model the step is made with: the controller's model is replaced by them first (``update_model``).  ``bounds``: likewise a dict
    under any of the names xmin, xmax, umin, umax, Dumin, Dumax, each [B, nx | nu] or unbatched [nx | nu] -- the constraint bounds the step is
    made with, differentiable too.  ``d`` [B, nx] or [B, Np, nx]: the affine term of the prediction model x+ = Ad x + Bd u + d the step is made
    with (``set_affine``; it stays in force afterwards), differentiable too; None: the controller's own, if it has one, no gradient.
    The rollouts below refuse a controller that has a term (NotImplementedError: the tapes do not carry it)."""
    names, tensors = _check_args('mpc_step', controller, params, bounds=bounds)
    if d is not None and (not hasattr(d, 'data_ptr') or not d.is_cuda):
        raise ValueError('mpc_step: d must be a device tensor [B, nx] or [B, Np, nx]')
    return _MPCStep.apply(controller, x, u_prev, xref, d, names, *tensors)


# ---- a closed-loop rollout as one differentiable operation (include/mpcqp_rollout.h, include/mpcqp_rollout_est.h, include_ext*/) ------------
_per = lambda v, shp: v.sum(dim=0) if len(shp) == 2 else v      # (an unbatched matrix input: summed over the batch)
# input of a rollout -> (the gradient of rollout_adjoint it is made from, how; its own shape is put on last)
_ROLLOUT_INPUTS = dict(
    x0=('lam', lambda v, shp: v[0]), w=('lam', lambda v, shp: v[1:]), xhat0=('eta', lambda v, shp: v[0]), v=('v', lambda v, shp: v),
    u_prev=('uminus1', lambda v, shp: v), xref=('xref', lambda v, shp: v.sum(dim=0)), C=('C', _per), L=('L', _per), Ap=('Ap', _per), Bp=('Bp', _per),
    d0=('d0', lambda v, shp: v),
    # (entries beyond the last one a solve could use were never in force: zeros)
    d=('d_traj', lambda v, shp: torch.cat([v[:shp[0]], v.new_zeros((max(shp[0] - v.shape[0], 0),) + tuple(v.shape[1:]))])))


def _model_paths(est, sched, follows, given_Ad=False, given_Bd=False):
    """Which gradients of ``rollout_adjoint`` add up, in this order, to the gradient of each input that is a model matrix -- a pure rule.
    Ad (Bd likewise) has up to three paths: the solves made under it ('Ad'), the estimator where there is one (``est``: 'Ae') and the plant
    where it follows the controller's model (``follows``: 'Ap').  Under a schedule (``sched``) that gave the matrix, entry e of ``Ad_traj``
    collects the three of the steps it was in force ('Ad_traj', 'Ae_traj', 'Ap_traj'), and ``params['Ad']``, the model the rollout began
    with, is left with the first solve's share; a matrix the schedule did not give never changed, so the parameter collects all of them,
    summed over the entries, as it does without a schedule."""
    paths = {}
    for m, given in (('A', given_Ad), ('B', given_Bd)):
        of = lambda suffix: [m + 'd' + suffix] + ([m + 'e' + suffix] if est else []) + ([m + 'p' + suffix] if follows else [])
        per_entry = bool(sched and given)
        paths[m + 'd_traj'] = of('_traj') if per_entry else []
        paths[m + 'd'] = [m + 'd'] if per_entry else of('')
    return paths


def _rollout_forward(ctx, fn, K, nsteps, inputs, names, params, hold=None, d_hold=None):
    """Forward of every form.  ``inputs``: forward's tensor inputs by name, in its order behind (K, nsteps[, hold]) -- keys of _ROLLOUT_INPUTS
    and, under a schedule (``hold``), 'Ad_traj', 'Bd_traj' and, with an estimator ('C' is among them), 'L_traj'.  ``update_model`` of the
    parameters, ``update(x0 or xhat0, u_prev, xref)`` with its solve (tape entry 0), then the taped loop of ``BatchProblem`` the options pick,
    and the controller's and the context's books.
    With an affine term (``d_hold``; (K, nsteps, hold, d_hold) stand before the inputs, ``hold`` None without a model schedule): 'd0', the term
    of that first solve (``set_affine`` before the update; None: the controller's own, or none), and 'd', the schedule of ``rollout_affine``."""
    x0 = inputs['x0']
    if not x0.is_cuda:
        raise ValueError('%s works on device tensors (x0 is on %s)' % (fn, x0.device))
    est, sched, aff = 'C' in inputs, hold is not None, d_hold is not None
    B, nx, nu = K.B, K.nx, K.nu
    with _ordered(K):
        _put_params(ctx, K, names, params)
        if aff and inputs['d0'] is not None:
            K.set_affine(_det(inputs['d0']).reshape(B, -1))
        xr = _det(inputs['xref'])
        K.update(_det(inputs['xhat0'] if est else x0), _det(inputs['u_prev']), None if xr is None else xr.reshape(B, -1))
        new = lambda rows, cols: torch.empty((rows, B, cols), dtype=torch.float64, device=x0.device)
        st, it = (torch.empty((nsteps, B), dtype=torch.int32, device=x0.device) for _ in range(2))
        X, U = new(nsteps + 1, nx), new(nsteps, nu)
        out, more = [X, U, st, it], {}
        if est:
            ny = int(inputs['C'].shape[-2])
            XH, Y = new(nsteps + 1, nx), new(nsteps, ny)
            out += [XH, Y]
            more['estimator'] = dict(C=_bc(inputs['C'], (B, ny, nx)), L=_bc(inputs['L'], (B, nx, ny)), x_true=_det(x0).clone(), v=_det(inputs['v']))
        if sched:
            nseg = ctx.nseg = (nsteps + hold - 1) // hold
            # [nseg, B, ., .] of the entries in force (entry e of an unbatched schedule is one model, one gain, for the whole batch)
            entries = lambda t: None if t is None else _det(t)[:nseg].reshape((nseg, -1) + tuple(t.shape[-2:])).expand((nseg, B) + tuple(t.shape[-2:])).contiguous()
            last = dict(Ad=entries(inputs['Ad_traj']), Bd=entries(inputs['Bd_traj']))
            more['model_traj'] = (last['Ad'], last['Bd'], hold)
            if est:
                more['L_traj'] = entries(inputs['L_traj'])
        if aff:
            d = _det(inputs['d'])
            more.update(d_traj=d.reshape(d.shape[0], B, -1), d_hold=d_hold)
        roll = getattr(K.prob, 'rollout_affine' if aff else 'rollout' + ('_tv' if sched else '') + ('_est' if est else ''))
        roll(nsteps, w=_det(inputs['w']), Ap=_bc(inputs['Ap'], (B, nx, nx)), Bp=_bc(inputs['Bp'], (B, nx, nu)), out=out, **more)
        for n, t in last.items() if sched else ():             # the controller is left with the last entry used: read back when somebody asks (update_model's way)
            if t is not None:
                K.__dict__.pop(n, None)
                K._on_device[n] = t[nseg - 1]
        K.solve_count += nsteps
        K.x0_rh, K.uminus1_rh, K._um1_on_device, K._u_last = (XH if est else X)[-1], U[-1], True, None
    ctx.K, ctx.count = K, K.prob.rollout_count
    ctx.fn, ctx.est, ctx.sched = fn, est, sched
    ctx.first = 4 if aff else 3 if sched else 2            # (K, nsteps[, hold[, d_hold]]) stand before the tensor inputs, ``names`` behind them
    ctx.inputs, ctx.shapes = tuple(inputs), tuple(None if t is None else tuple(t.shape) for t in inputs.values())
    ctx.status, ctx.iters = st, it
    return (X, XH, Y, U) if est else (X, U)


def _rollout_backward(ctx, **seeds):
    """Backward of every form: one ``rollout_adjoint`` call, with its ``seeds`` by name, for exactly the gradients torch needs."""
    K, fn, inputs, est, sched = ctx.K, ctx.fn, ctx.inputs, ctx.est, ctx.sched
    if K.prob.rollout_count != ctx.count:
        raise RuntimeError('%s: the controller has been rolled out again since this forward (rollout %d then, %d now); '
                           'its tape is no longer the one to differentiate.' % (fn, ctx.count, K.prob.rollout_count))
    first = ctx.first
    ni = first + len(inputs)
    need = {n: bool(v) and shp is not None for n, v, shp in zip(inputs, ctx.needs_input_grad[first:ni], ctx.shapes)}
    shape = dict(zip(inputs, ctx.shapes))
    traj = [n for n in inputs if n.endswith('_traj')]
    unbatched = lambda n: len(shape[n]) == (3 if n in traj else 2)
    # (under a schedule rollout_adjoint puts these together from per-entry buffers, and batch_sum sums them too)
    split = [n for n in traj + ['Ap', 'Bp', 'L'] if need.get(n)] if sched else []
    # (the terms of an affine rollout are per instance, and batch_sum would sum their gradients too)
    pneed, shared, batch_sum = _param_want(ctx, ctx.needs_input_grad[ni + 1:], [unbatched(n) for n in split] + [False for n in ('d0', 'd') if need.get(n)])
    if not any(need.values()) and not pneed:
        return (None,) * (ni + 1 + len(ctx.names))
    paths = _model_paths(est, sched, shape['Ap'] is None, shape.get('Ad_traj') is not None, shape.get('Bd_traj') is not None)
    paths['L_traj'] = ['L_traj']
    want = [_ROLLOUT_INPUTS[n][0] for n in inputs if need[n] and n not in traj]
    want += [g for n in traj if need[n] for g in paths[n]] + [g for n in pneed for g in paths.get(n, [n])]
    with _ordered(K):
        res = K.prob.rollout_adjoint(want=list(dict.fromkeys(want)), batch_sum=batch_sum, **{k: g.to(torch.float64).contiguous() for k, g in seeds.items()})
    grads = []
    for n in inputs:
        v = None
        if need[n] and n in traj:                          # entry e: its paths added up, then the batch where the schedule is unbatched
            v = res[paths[n][0]]
            for g in paths[n][1:]:
                v = v + res[g]
            v = (v.sum(dim=1) if unbatched(n) else v)[:ctx.nseg]
            if shape[n][0] > ctx.nseg:                     # entries beyond ceil(nsteps / hold) were never in force
                v = torch.cat([v, v.new_zeros((shape[n][0] - ctx.nseg,) + tuple(v.shape[1:]))])
            v = v.reshape(shape[n])
        elif need[n]:
            v = _ROLLOUT_INPUTS[n][1](res[_ROLLOUT_INPUTS[n][0]], shape[n]).reshape(shape[n])
        grads.append(v)
    return (None,) * first + tuple(grads) + (None,) + tuple(_param_grads(ctx, res, pneed, shared, batch_sum, paths, sched))


class _MPCRollout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, K, nsteps, x0, u_prev, xref, w, Ap, Bp, names, *params):
        return _rollout_forward(ctx, 'mpc_rollout', K, nsteps, dict(x0=x0, u_prev=u_prev, xref=xref, w=w, Ap=Ap, Bp=Bp), names, params)

    @staticmethod
    def backward(ctx, grad_X, grad_U):
        return _rollout_backward(ctx, g_x=grad_X, g_u=grad_U)


def mpc_rollout(controller, x0, nsteps, u_prev=None, xref=None, w=None, Ap=None, Bp=None, params=None, bounds=None):
    """``(X [K+1,B,nx], U [K,B,nu])`` of ``nsteps`` = K closed-loop steps of a set-up ``BatchMPCController`` from ``x0`` [B,nx] against the
    plant x_{k+1} = Ap x_k + Bp u_k + w[k] (``Ap`` / ``Bp`` None: the controller's own Ad, Bd; ``w`` [K,B,nx] or None), on ONE controller:
    forward is ``update_model(solve=False, **params)`` where given, ``update(x0, u_prev, xref)`` with its solve, then
    ``BatchMPCController.rollout``'s device loop with a tape (mpcqp_rollout); backward is ONE ``mpcqp_rollout_adjoint`` call with
    ``G_x = grad_X``, ``G_u = grad_U`` -- one reverse sweep over the tape on the device, which factors the active-set system of a step only
    where its active set differs from the step's behind it.  Differentiable with respect to ``x0``, ``u_prev``, ``xref`` (constant over
    the rollout), ``w``, ``Ap``, ``Bp`` ([B, ., .] or unbatched) and ``params`` (as in ``mpc_step``; with ``Ap`` / ``Bp`` None the gradients
    of ``params['Ad']`` / ``['Bd']`` include the plant path).  A step whose solve does not end 'solved' applies ``u_failure`` = uref and
    passes the gradient through the plant alone.  The tape is a copy: stepping or solving the controller between forward and backward is
    fine, another rollout is not -- the backward then raises.  ``bounds`` as in ``mpc_step``: constant over the rollout, their gradient the
    sum over its steps."""
    names, tensors = _check_args('mpc_rollout', controller, params, Ap, Bp, bounds)
    return _MPCRollout.apply(controller, int(nsteps), x0, u_prev, xref, w, Ap, Bp, names, *tensors)


class _MPCRolloutTV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, K, nsteps, hold, x0, u_prev, xref, w, Ap, Bp, Ad_traj, Bd_traj, names, *params):
        inputs = dict(x0=x0, u_prev=u_prev, xref=xref, w=w, Ap=Ap, Bp=Bp, Ad_traj=Ad_traj, Bd_traj=Bd_traj)
        return _rollout_forward(ctx, 'mpc_rollout_tv', K, nsteps, inputs, names, params, hold)

    @staticmethod
    def backward(ctx, grad_X, grad_U):
        return _rollout_backward(ctx, g_x=grad_X, g_u=grad_U)


class _MPCRolloutAffine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, K, nsteps, hold, d_hold, x0, u_prev, xref, w, Ap, Bp, Ad_traj, Bd_traj, d0, d, names, *params):
        inputs = dict(x0=x0, u_prev=u_prev, xref=xref, w=w, Ap=Ap, Bp=Bp, Ad_traj=Ad_traj, Bd_traj=Bd_traj, d0=d0, d=d)
        return _rollout_forward(ctx, 'mpc_rollout_affine', K, nsteps, inputs, names, params, hold, d_hold)

    @staticmethod
    def backward(ctx, grad_X, grad_U):
        return _rollout_backward(ctx, g_x=grad_X, g_u=grad_U)


def mpc_rollout_affine(controller, x0, nsteps, d, d_hold=1, d0=None, Ad_traj=None, Bd_traj=None, hold=None, u_prev=None, xref=None, w=None, Ap=None, Bp=None,
                       params=None, bounds=None, offset_in_plant=False):
    """``mpc_rollout`` / ``mpc_rollout_tv`` with an affine term in the prediction model, x+ = Ad x + Bd u + d: ``(X [K+1,B,nx], U [K,B,nu])`` of
    ``nsteps`` = K closed-loop steps in which the solve after step k uses entry ``k // d_hold`` of ``d`` [nent,B,nx] or [nent,B,Np,nx] (nent >=
    ceil(K / d_hold)), as ``BatchMPCController.run(d_traj=, d_hold=)`` does; the first solve uses ``d0`` [B,nx] or [B,Np,nx] in the shape of the
    entries (None: the controller's own term, or none).  With ``Ad_traj`` / ``Bd_traj`` and ``hold`` the loop runs under a model schedule too, as
    ``mpc_rollout_tv``: one entry (A_e, B_e, c_e) per relinearisation.  Forward is ``update_model``, ``set_affine(d0)``, ``update`` with its solve,
    then ONE ``mpcqp_rollout_affine``; backward is ONE ``mpcqp_rollout_adjoint_affine`` (include_ext5/mpcqp_rollout_affine.h).  Differentiable
    with respect to ``d``, ``d0`` and everything those two layers differentiate.  The plant does not get the offset, unless ``offset_in_plant``:
    then entry ``k // d_hold`` of a one-row ``d`` is added to ``w[k]`` (in torch: its gradient arrives through ``w``) -- a relinearised plant.
    The controller is left with the last entry used."""
    names, tensors = _check_args('mpc_rollout_affine', controller, params, Ap, Bp, bounds)
    nsteps, d_hold = int(nsteps), int(d_hold)
    if d_hold < 1:
        raise ValueError('mpc_rollout_affine: d_hold must be >= 1')
    nent = (nsteps + d_hold - 1) // d_hold
    if not hasattr(d, 'data_ptr') or not d.is_cuda or d.dim() not in (3, 4) or d.shape[0] < nent or d.shape[1] != controller.B:
        raise ValueError('mpc_rollout_affine: d must be a device tensor [nent, B, nx] or [nent, B, Np, nx] with nent >= ceil(nsteps / d_hold)')
    if d0 is not None and (not hasattr(d0, 'data_ptr') or not d0.is_cuda or d0.numel() != d[0].numel()):
        raise ValueError('mpc_rollout_affine: d0 must be a device tensor in the shape of an entry of d')
    sched = Ad_traj is not None or Bd_traj is not None
    if sched and hold is None:
        raise ValueError('mpc_rollout_affine: a model schedule needs its hold')
    if sched:
        nseg = (nsteps + int(hold) - 1) // int(hold)
        for n, t in (('Ad_traj', Ad_traj), ('Bd_traj', Bd_traj)):
            if t is not None and (not hasattr(t, 'data_ptr') or not t.is_cuda or t.dim() not in (3, 4) or t.shape[0] < nseg):
                raise ValueError('mpc_rollout_affine: %s must be a device tensor [nseg, B, ., .] or [nseg, ., .] with nseg >= ceil(nsteps / hold)' % n)
    if offset_in_plant:
        if d.numel() != d.shape[0] * controller.B * controller.nx:
            raise ValueError('mpc_rollout_affine: offset_in_plant is for a one-row term [nent, B, nx] (the plant steps once: which stage of an Np-row term is its own is not said)')
        off = d.reshape(d.shape[0], controller.B, controller.nx).repeat_interleave(d_hold, dim=0)[:nsteps]
        w = off if w is None else w + off
    return _MPCRolloutAffine.apply(controller, nsteps, int(hold) if sched else None, d_hold, x0, u_prev, xref, w, Ap, Bp, Ad_traj, Bd_traj, d0, d, names, *tensors)


def mpc_rollout_tv(controller, x0, nsteps, Ad_traj, Bd_traj, hold, u_prev=None, xref=None, w=None, Ap=None, Bp=None, params=None, bounds=None):
    """``mpc_rollout`` under a model schedule: ``(X [K+1,B,nx], U [K,B,nu])`` of ``nsteps`` = K closed-loop steps in which entry ``k // hold``
    of ``Ad_traj`` [nseg,B,nx,nx] / ``Bd_traj`` [nseg,B,nx,nu] (or unbatched [nseg,nx,nx] / [nseg,nx,nu]; either may be None, not both;
    nseg >= ceil(K / hold)) replaces the controller's model at the start of step k, as ``BatchMPCController.run(model_traj=)`` does -- a
    controller tracking a relinearised plant.  Forward is ``update_model(solve=False, **params)`` where given, ``update(x0, u_prev, xref)``
    with its solve (made under the model the controller holds then: tape entry 0), then ONE ``mpcqp_rollout_tv``; backward is ONE
    ``mpcqp_rollout_adjoint_tv`` on torch's current stream.  Differentiable with respect to every tensor argument: the gradient of
    ``Ad_traj[e]`` is that of the solves made under entry e plus, where ``Ap`` is None (the plant follows the schedule), that of the plant
    steps it was in force; ``params['Ad']`` is the model the rollout begins with and gets the first solve's share (and, where the schedule
    leaves Ad alone, everything).  An unbatched schedule's gradient is the sum over the batch, formed on the device.  Everything else as
    in ``mpc_rollout``."""
    names, tensors = _check_args('mpc_rollout_tv', controller, params, Ap, Bp, bounds)
    if Ad_traj is None and Bd_traj is None:
        raise ValueError('mpc_rollout_tv: give Ad_traj, Bd_traj or both (mpc_rollout is the loop on one model)')
    nseg = (int(nsteps) + int(hold) - 1) // int(hold)
    for n, t in (('Ad_traj', Ad_traj), ('Bd_traj', Bd_traj)):
        if t is not None and (not hasattr(t, 'data_ptr') or not t.is_cuda or t.dim() not in (3, 4) or t.shape[0] < nseg):
            raise ValueError('mpc_rollout_tv: %s must be a device tensor [nseg, B, ., .] or [nseg, ., .] with nseg >= ceil(nsteps / hold)' % n)
    return _MPCRolloutTV.apply(controller, int(nsteps), int(hold), x0, u_prev, xref, w, Ap, Bp, Ad_traj, Bd_traj, names, *tensors)


class _MPCRolloutEst(torch.autograd.Function):
    @staticmethod
    def forward(ctx, K, nsteps, x0, xhat0, C, L, v, u_prev, xref, w, Ap, Bp, names, *params):
        inputs = dict(x0=x0, xhat0=xhat0, C=C, L=L, v=v, u_prev=u_prev, xref=xref, w=w, Ap=Ap, Bp=Bp)
        return _rollout_forward(ctx, 'mpc_rollout_est', K, nsteps, inputs, names, params)

    @staticmethod
    def backward(ctx, grad_X, grad_XH, grad_Y, grad_U):
        return _rollout_backward(ctx, g_x=grad_X, g_u=grad_U, g_xhat=grad_XH, g_y=grad_Y)


def mpc_rollout_est(controller, x0, xhat0, nsteps, C, L, v=None, u_prev=None, xref=None, w=None, Ap=None, Bp=None, params=None, bounds=None):
    """``(X [K+1,B,nx], Xhat [K+1,B,nx], Y [K,B,ny], U [K,B,nu])`` of ``nsteps`` = K steps of the OUTPUT-FEEDBACK loop of a set-up
    ``BatchMPCController``: the plant x_{k+1} = Ap x_k + Bp u_k + w[k] starts at ``x0`` [B,nx], the controller sees the estimate only, which
    starts at ``xhat0`` [B,nx] and follows xhat_{k+1} = Ad (xhat_k + L (y_k - C xhat_k)) + Bd u_k with y_k = C x_k + v[k] (``C`` [B,ny,nx] or
    [ny,nx], ``L`` [B,nx,ny] or [nx,ny], ``v`` [K,B,ny] or None).  Forward is ``update_model(solve=False, **params)`` where given,
    ``update(xhat0, u_prev, xref)`` with its solve, then the device loop with a tape (mpcqp_rollout_est); backward is ONE
    ``mpcqp_rollout_adjoint_est`` call with the four seeds ``grad_X, grad_Xhat, grad_Y, grad_U``.  Differentiable with respect to ``x0``,
    ``xhat0``, ``C``, ``L``, ``v``, ``u_prev``, ``xref``, ``w``, ``Ap``, ``Bp`` and ``params`` (as in ``mpc_rollout``); the gradients of
    ``params['Ad']`` / ``['Bd']`` include the estimator's path and, with ``Ap`` / ``Bp`` None, the plant's.  ``mpc_rollout`` is the loop
    without an estimator.  ``bounds`` as in ``mpc_rollout``."""
    names, tensors = _check_args('mpc_rollout_est', controller, params, Ap, Bp, bounds)
    for n, t in (('C', C), ('L', L)):
        if not hasattr(t, 'data_ptr') or not t.is_cuda or t.dim() not in (2, 3):
            raise ValueError('mpc_rollout_est: %s must be a device tensor [B, ., .] or [., .]' % n)
    return _MPCRolloutEst.apply(controller, int(nsteps), x0, xhat0, C, L, v, u_prev, xref, w, Ap, Bp, names, *tensors)


class _MPCRolloutTVEst(torch.autograd.Function):
    @staticmethod
    def forward(ctx, K, nsteps, hold, x0, xhat0, C, L, v, u_prev, xref, w, Ap, Bp, Ad_traj, Bd_traj, L_traj, names, *params):
        inputs = dict(x0=x0, xhat0=xhat0, C=C, L=L, v=v, u_prev=u_prev, xref=xref, w=w, Ap=Ap, Bp=Bp, Ad_traj=Ad_traj, Bd_traj=Bd_traj, L_traj=L_traj)
        return _rollout_forward(ctx, 'mpc_rollout_tv_est', K, nsteps, inputs, names, params, hold)

    @staticmethod
    def backward(ctx, grad_X, grad_XH, grad_Y, grad_U):
        return _rollout_backward(ctx, g_x=grad_X, g_u=grad_U, g_xhat=grad_XH, g_y=grad_Y)


def mpc_rollout_tv_est(controller, x0, xhat0, nsteps, Ad_traj, Bd_traj, hold, C, L=None, L_traj=None, v=None, u_prev=None, xref=None, w=None, Ap=None, Bp=None,
                       params=None, bounds=None):
    """``mpc_rollout_est`` under a model schedule: ``(X [K+1,B,nx], Xhat [K+1,B,nx], Y [K,B,ny], U [K,B,nu])`` of ``nsteps`` = K steps of the
    output-feedback loop in which entry ``k // hold`` of ``Ad_traj`` / ``Bd_traj`` (as in ``mpc_rollout_tv``) replaces the model at the start of
    step k -- for the controller, for the estimator xhat_{k+1} = Ad_e (xhat_k + L_e (y_k - C xhat_k)) + Bd_e u_k and, with ``Ap`` / ``Bp`` None,
    for the plant -- as ``BatchMPCController.run(estimator=, model_traj=, L_traj=)`` does.  Exactly one of ``L`` ([B,nx,ny] or [nx,ny]: one
    gain throughout) and ``L_traj`` ([nseg,B,nx,ny] or [nseg,nx,ny]: a gain per entry, e.g. ``kalman_gain(Ad_traj[e], C, Qn, Rn)``) is given.
    Forward is ``update_model(solve=False, **params)`` where given, ``update(xhat0, u_prev, xref)`` with its solve, then ONE
    ``mpcqp_rollout_tv_est`` (include_ext2/mpcqp_rollout_tv_est.h); backward is ONE ``mpcqp_rollout_adjoint_tv_est`` with the four seeds.
    Differentiable with respect to every tensor argument: the gradient of ``Ad_traj[e]`` is that of the solves made under entry e plus that of
    the estimator steps it was in force plus, where ``Ap`` is None, that of the plant steps; ``params['Ad']`` is the model the rollout
    begins with and gets the first solve's share (and, where the schedule leaves Ad alone, everything).  An unbatched schedule's or gain
    schedule's gradient is the sum over the batch.  Everything else as in ``mpc_rollout_est`` and ``mpc_rollout_tv``."""
    names, tensors = _check_args('mpc_rollout_tv_est', controller, params, Ap, Bp, bounds)
    if Ad_traj is None and Bd_traj is None:
        raise ValueError('mpc_rollout_tv_est: give Ad_traj, Bd_traj or both (mpc_rollout_est is the loop on one model)')
    if (L is None) == (L_traj is None):
        raise ValueError('mpc_rollout_tv_est: give exactly one of L and L_traj')
    nseg = (int(nsteps) + int(hold) - 1) // int(hold)
    for n, t in (('Ad_traj', Ad_traj), ('Bd_traj', Bd_traj), ('L_traj', L_traj)):
        if t is not None and (not hasattr(t, 'data_ptr') or not t.is_cuda or t.dim() not in (3, 4) or t.shape[0] < nseg):
            raise ValueError('mpc_rollout_tv_est: %s must be a device tensor [nseg, B, ., .] or [nseg, ., .] with nseg >= ceil(nsteps / hold)' % n)
    for n, t in (('C', C), ('L', L)):
        if t is not None and (not hasattr(t, 'data_ptr') or not t.is_cuda or t.dim() not in (2, 3)):
            raise ValueError('mpc_rollout_tv_est: %s must be a device tensor [B, ., .] or [., .]' % n)
    if C is None:
        raise ValueError('mpc_rollout_tv_est: C is needed')
    return _MPCRolloutTVEst.apply(controller, int(nsteps), int(hold), x0, xhat0, C, L, v, u_prev, xref, w, Ap, Bp, Ad_traj, Bd_traj, L_traj, names, *tensors)


# ---- the discrete algebraic Riccati equation as a differentiable operation (include/mpcqp_riccati.h) ------------------------------------
class _Dare(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gain_form, A, B, Q, R):
        from . import riccati
        X, K, status, _, _ = riccati.dare(A, B, Q, R, gain_form=gain_form)
        ctx.save_for_backward(A, B, Q, R, X, K)
        ctx.gain_form, ctx.status = gain_form, status
        return X, K, status

    @staticmethod
    def backward(ctx, grad_X, grad_K, _):
        from . import riccati
        A, B, Q, R, X, K = ctx.saved_tensors
        want = [n for n, need in zip('ABQR', ctx.needs_input_grad[1:]) if need]
        if not want:
            return (None,) * 5
        g = riccati.dare_adjoint(A, B, Q, R, X, K, status=ctx.status, G_X=grad_X, G_K=grad_K, gain_form=ctx.gain_form, want=want)
        # (an unbatched input beside batched ones: one matrix shared by the batch, its gradient the sum over it)
        return (None,) + tuple(None if n not in g else (g[n].sum(dim=0) if p.dim() == 2 and g[n].dim() == 3 else g[n]) for n, p in zip('ABQR', (A, B, Q, R)))


def _riccati_args(fn, **mats):
    for n, t in mats.items():
        if not hasattr(t, 'data_ptr') or not t.is_cuda or t.dim() not in (2, 3):
            raise ValueError('%s: %s must be a device tensor [B, ., .] or [., .]' % (fn, n))


def dare(A, B, Q, R, gain_form=0):
    """``(X, K)`` of X = A'XA - A'XB (R + B'XB)^-1 B'XA + Q for device tensors [B, ., .] or unbatched [., .] (``pympc_amd.riccati.dare``):
    forward is ONE mpcqp_dare call, backward ONE mpcqp_dare_adjoint call, both on torch's current stream.  ``gain_form`` 0: K = (R + B'XB)^-1
    B'XA, 1: (R + B'XB)^-1 B'X.  Differentiable with respect to all four; the gradients of Q and R are those of a symmetric perturbation, an
    unbatched input beside batched ones gets the sum over the batch, an instance that did not converge returns zeros and contributes a zero
    gradient.  ``X.status`` ( = ``K.status``): the int32 status per instance (1 converged, 0 not, -1 not positive definite)."""
    _riccati_args('dare', A=A, B=B, Q=Q, R=R)
    X, K, status = _Dare.apply(int(gain_form), A, B, Q, R)
    X.status = K.status = status
    return X, K


def kalman_gain(A, C, Qn, Rn, type='filter'):
    """``(L, P)`` of the stationary Kalman filter ('filter': L = P C' (C P C' + Rn)^-1) or predictor ('predictor': L = A P C' (C P C' + Rn)^-1)
    of x+ = A x + w, y = C x + v -- the meaning of ``pympc_amd.kalman.kalman_design_simple`` -- as ``dare`` of the dual problem
    (A', C', Qn, Rn): differentiable with respect to A, C and the noise covariances Qn, Rn.  L is [.., nx, ny]; ``L.status``, ``P.status``
    as in ``dare``."""
    if type not in ('filter', 'predictor'):
        raise ValueError("Unknown Kalman design type. Specify either filter or predictor!")
    _riccati_args('kalman_gain', A=A, C=C, Qn=Qn, Rn=Rn)
    P, G = dare(A.transpose(-1, -2).contiguous(), C.transpose(-1, -2).contiguous(), Qn, Rn, gain_form=1 if type == 'filter' else 0)
    L = G.transpose(-1, -2).contiguous()
    L.status = P.status
    return L, P


# ---- the Riccati difference equation as a differentiable operation (include_ext3/mpcqp_riccati_traj.h) ---------------------------------
class _Dre(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gain_form, a_traj, b_traj, T, A, B, Q, R, X0):
        from . import riccati
        X, K, status, bad = riccati.dre_flagged(A, a_traj, B, b_traj, Q, R, X0, gain_form=gain_form, T=T)
        ctx.save_for_backward(A, B, Q, R, X0, X)
        ctx.conf, ctx.status = (gain_form, a_traj, b_traj, T), status
        ctx.mark_non_differentiable(status, bad)
        return X, K, status, bad

    @staticmethod
    def backward(ctx, grad_X, grad_K, _s, _b):
        from . import riccati
        A, B, Q, R, X0, X = ctx.saved_tensors
        gain_form, a_traj, b_traj, T = ctx.conf
        names = ('A', 'B', 'Q', 'R', 'X0')
        want = [n for n, need in zip(names, ctx.needs_input_grad[4:]) if need]
        if not want:
            return (None,) * 9
        g = riccati.dre_adjoint_flagged(A, a_traj, B, b_traj, Q, R, X0, X, status=ctx.status, G_X=grad_X, G_K=grad_K, gain_form=gain_form, T=T, want=want)
        # (an unbatched input beside batched ones: one matrix or trajectory shared by the batch, its gradient the sum over it)
        out = []
        for n, p, tr in zip(names, (A, B, Q, R, X0), (a_traj, b_traj, False, False, False)):
            out.append(None if n not in g else (g[n].sum(dim=1 if tr else 0) if g[n].dim() == p.dim() + 1 else g[n]))
        return (None,) * 4 + tuple(out)


def _dre_flagged(A, a_traj, B, b_traj, Q, R, X0, gain_form=0, T=None, stream=None):
    """``riccati.dre_flagged`` as the differentiable operation (``stream`` is torch's current one)."""
    return _Dre.apply(int(gain_form), bool(a_traj), bool(b_traj), None if T is None else int(T), A, B, Q, R, X0)


def _traj_args(fn, mats, trajs):
    for n, t in mats.items():
        if not hasattr(t, 'data_ptr') or not t.is_cuda or t.dim() not in (2, 3):
            raise ValueError('%s: %s must be a device tensor [B, ., .] or [., .]' % (fn, n))
    for n, t in trajs.items():
        if not hasattr(t, 'data_ptr') or not t.is_cuda or t.dim() not in (2, 3, 4):
            raise ValueError('%s: %s must be a device tensor, one matrix ([B, ., .] or [., .]) or a trajectory ([T, B, ., .] or [T, ., .])' % (fn, n))


def dre(A, B, Q, R, X0, gain_form=0, T=None):
    """``(X_traj, K_traj)`` of the Riccati difference equation from X0 over T steps for device tensors (``pympc_amd.riccati.dre``, which
    says how A and B are read as one matrix or as a trajectory): forward is ONE mpcqp_dre call, backward ONE mpcqp_dre_adjoint call, both on
    torch's current stream.  Differentiable with respect to A, B, Q, R and X0; the gradients of Q, R and X0 are those of a symmetric
    perturbation, a trajectory gets a gradient per entry and one matrix the sum over the steps, an unbatched input beside batched ones the
    sum over the batch; an instance that did not run through returns zeros and contributes a zero gradient.  ``X_traj.status``
    ( = ``K_traj.status``) and ``.first_bad``: per instance, as in ``riccati.dre``."""
    from . import riccati
    _traj_args('dre', dict(Q=Q, R=R, X0=X0), dict(A=A, B=B))
    a_traj, b_traj = riccati.traj_flags('dre', A, B, (Q, R, X0))
    X, K, status, bad = _dre_flagged(A, a_traj, B, b_traj, Q, R, X0, gain_form=gain_form, T=T)
    X.status = K.status = status
    X.first_bad = K.first_bad = bad
    return X, K


def kalman_gain_traj(A_traj, C, Qn, Rn, P0, hold=1):
    """``(L_traj [nentries, B, nx, ny], P_traj [nentries + 1, B, nx, nx])`` of the Kalman filter of a time-varying system, with the meaning
    and the indexing of ``pympc_amd.riccati.kalman_gain_traj`` (entry e: the gain and the covariance at the first step of schedule entry
    e; ``mpc_rollout_tv_est(.., L_traj=L_traj)`` under the same ``hold`` is that filter): ONE mpcqp_dre call forward, ONE
    mpcqp_dre_adjoint call backward.  Differentiable with respect to every entry of ``A_traj``, C, the noise covariances Qn, Rn and the
    initial covariance P0.  ``L_traj.status``, ``P_traj.status`` as in ``dre``."""
    from . import riccati
    _traj_args('kalman_gain_traj', dict(C=C, Qn=Qn, Rn=Rn, P0=P0), {})
    if not hasattr(A_traj, 'data_ptr') or not A_traj.is_cuda or A_traj.dim() not in (3, 4):
        raise ValueError('kalman_gain_traj: A_traj must be a device tensor [nentries, B, nx, nx] or [nentries, nx, nx]')
    L, P, status = riccati._dre_dual(_dre_flagged, A_traj, C, Qn, Rn, P0, riccati._hold(hold), None)
    L.status = P.status = status
    return L, P
