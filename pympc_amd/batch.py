"""Batched controllers: B independent ``MPCController``s of identical (nx, nu, Np, Nc) solved in
one kernel launch per control step (additive surface named in SURVEY.md section 8b).

Semantics per instance are those of the reference class (pyMPC/mpc.py): ``setup()`` builds and
cold-solves, ``update(x, u=None, xref=None)`` refreshes q/l/u and warm-solves, ``output()`` returns
the first optimal input, or ``uref`` for instances whose status is not 'solved' (mpc.py:301-304),
and remembers it as the next u_{-1} (mpc.py:330).
"""
import numpy as np

from .solver import BatchProblem


def _est_dict(estimator):
    """What ``BatchProblem`` takes of a ``BatchLinearStateEstimator`` (None: state feedback)."""
    if estimator is None:
        return None
    return dict(C=estimator.C, L=estimator.L, x_true=estimator.x_true, v=getattr(estimator, 'v', None))


class BatchMPCController:
    def __init__(self, Ad, Bd, Np=20, Nc=None, x0=None, xref=None, uref=None, uminus1=None,
                 Qx=None, QxN=None, Qu=None, QDu=None,
                 xmin=None, xmax=None, umin=None, umax=None, Dumin=None, Dumax=None,
                 eps_feas=1e6, eps_rel=1e-3, eps_abs=1e-3, device=0, stream=None, SOFT_ON=True, **solver_settings):
        Ad = np.asarray(Ad, dtype=float)
        Bd = np.asarray(Bd, dtype=float)
        if Ad.ndim != 3 or Ad.shape[1] != Ad.shape[2]:
            raise ValueError("Ad should be a stack of square matrices of dimension (B,nx,nx)!")
        B, nx = Ad.shape[0], Ad.shape[1]
        if Bd.ndim != 3 or Bd.shape[0] != B or Bd.shape[1] != nx:
            raise ValueError("Bd should be a stack of matrices of dimension (B,nx,nu)!")
        nu = Bd.shape[2]
        if not Np > 1:
            raise ValueError("Np should be > 1!")
        if Nc is not None and not Nc <= Np:
            raise ValueError("Nc should be <= Np!")
        self.B, self.nx, self.nu, self.Np, self.Nc = B, nx, nu, Np, (Np if Nc is None else Nc)

        def bc(a, shape, default):
            if a is None:
                a = default
            return np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=float), shape))

        inf = np.inf
        self.Ad, self.Bd = Ad, Bd
        self.x0 = bc(x0, (B, nx), 0.0)
        self.uref = bc(uref, (B, nu), 0.0)
        self.uminus1 = bc(uminus1, (B, nu), self.uref)
        if xref is None:
            self.xref = np.zeros((B, nx))
        else:
            xref = np.asarray(xref, dtype=float)
            if xref.shape[-1] != nx:
                raise ValueError("xref should be (B,nx) or (B,Np+1,nx)!")
            self.xref = bc(xref, (B, Np + 1, nx) if (xref.ndim == 3 or (xref.ndim == 2 and xref.shape[0] == Np + 1 and B != Np + 1)) else (B, nx), None)
        self.Qx = bc(Qx, (B, nx, nx), 0.0)
        self.QxN = bc(QxN, (B, nx, nx), self.Qx)
        self.Qu = bc(Qu, (B, nu, nu), 0.0)
        self.QDu = bc(QDu, (B, nu, nu), 0.0)
        self.xmin = bc(xmin, (B, nx), -inf)
        self.xmax = bc(xmax, (B, nx), inf)
        self.umin = bc(umin, (B, nu), -inf)
        self.umax = bc(umax, (B, nu), inf)
        self.Dumin = bc(Dumin, (B, nu), -inf)
        self.Dumax = bc(Dumax, (B, nu), inf)
        self.eps_feas = bc(eps_feas, (B, 1), None)
        self.eps_rel, self.eps_abs = eps_rel, eps_abs
        self.u_failure = self.uref
        self.device, self.stream = device, stream
        self.solver_settings = dict(solver_settings)
        self.SOFT_ON = bool(SOFT_ON)           # pyMPC's hidden switch (mpc.py:237): False = hard state box, no slack variables
        self.prob = None
        self.uminus1_rh = None
        self.x0_rh = None
        self._u_last = None
        self._status = None
        # does the device copy of u_{-1} equal self.uminus1_rh?  output() moves the host value on (mpc.py:330) without
        # touching the device; setup()/update() upload it, step()/run() leave the applied input on the device themselves
        self._um1_on_device = False
        self._on_device = {}                      # model fields update_model() got as device tensors and nobody has read on the host since
        self.solve_count = 0                      # solves launched so far (pympc_amd.torch_layer: has the solution moved on since a forward?)

    def __getattr__(self, name):
        """A model field last given to ``update_model`` as a device tensor: its host copy is made on the first read, not per update."""
        dev = self.__dict__.get('_on_device', {})
        if name == 'u_failure' and 'uref' in dev:
            return self.uref
        if name in dev:
            v = np.ascontiguousarray(dev.pop(name).cpu().numpy(), dtype=float)
            setattr(self, name, v)
            if name == 'uref':
                self.u_failure = v
            return v
        raise AttributeError(name)

    def setup(self, solve=True):
        self.x0_rh = self.x0.copy()
        self.uminus1_rh = self.uminus1.copy()
        # same kwarg swap as the reference (mpc.py:266)
        st = dict(warm_start=True, eps_abs=self.eps_rel, eps_rel=self.eps_abs, soft_constraints=int(self.SOFT_ON))
        st.update(self.solver_settings)
        self.prob = BatchProblem(self.B, self.nx, self.nu, self.Np, self.Nc, device=self.device, stream=self.stream, **st)
        self.prob.setup(self.Ad, self.Bd, self.Qx, self.QxN, self.Qu, self.QDu, self.xmin, self.xmax,
                        self.umin, self.umax, self.Dumin, self.Dumax, self.uref, self.eps_feas,
                        self.x0_rh, self.uminus1_rh, self.xref)
        self._um1_on_device = True
        if solve:
            self.solve()

    def share_factor(self):
        """One model, many states (test_scripts/example_mpc_function.py:105-111): after ``setup()`` of a batch whose instances all carry the same model, every
        instance whose factorization inputs equal instance 0's solves with ONE shared copy of its KKT factor (``mpcqp_share_factor``); scatter the states with
        ``update()`` afterwards.  Results do not change; returns how many instances share (0 on the register-resident backends)."""
        return self.prob.share_factor()

    def update_model(self, solve=True, **fields):
        """New model data for the batch in use (``BatchProblem.update_model``): any of Ad, Bd, Qx, QxN, Qu, QDu, xmin, xmax, umin, umax, Dumin,
        Dumax, uref, eps_feas, broadcast to the batch like the constructor's arguments (numpy, or torch device tensors, which go down without a
        round trip through the host; the attributes stay numpy arrays, copied back when they are next read);
        what is not given keeps its value.  The device
        re-equilibrates, refactors and keeps every instance's iterate; ``solve=True`` then warm-solves like ``update``."""
        if self.prob is None:
            raise RuntimeError('update_model() needs a controller that has been set up; before setup() assign the attributes')
        shapes = self.prob._model_shapes()
        new = {}
        for k, v in fields.items():
            if k not in shapes:
                raise TypeError('unknown model field %r' % k)
            if v is not None and hasattr(v, 'data_ptr') and v.is_cuda:
                new[k] = v.detach().expand(shapes[k])     # (a torch device tensor goes down as it is, without a round trip through the host)
            elif v is not None:
                new[k] = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=float), shapes[k]))      # (ValueError if it does not fit, like the constructor)
        if not new:
            raise ValueError('update_model needs at least one model field')
        for k, v in new.items():
            if hasattr(v, 'data_ptr'):            # the host attribute stays a numpy array: copied from the device when somebody reads it (__getattr__)
                self.__dict__.pop(k, None)
                self._on_device[k] = v
            else:
                self._on_device.pop(k, None)
                setattr(self, k, v)
        if 'uref' in new:
            self.__dict__.pop('u_failure', None)  # (read through __getattr__: it is uref)
            if 'uref' not in self._on_device:
                self.u_failure = self.uref
        if not self._um1_on_device:               # output() moved u_{-1} on: the rho vector is built from the bounds as update() would leave them
            self.prob.update(None, self.uminus1_rh, None)
            self._um1_on_device = True
        self.prob.update_model(**new)
        if solve:
            self.solve()

    def set_affine(self, d):
        """The affine term of every instance's prediction model, x_{k+1} = Ad x_k + Bd u_k + d_k (``BatchProblem.set_affine``, include_ext4/mpcqp_affine.h):
        ``d`` [B, nx] (one offset for every stage) or [B, Np, nx] (row k: the step k -> k+1), numpy or a torch device tensor; ``None`` clears
        it.  It stays in force across update(), step(), run() and update_model() until it is replaced or cleared; setup() clears it."""
        if self.prob is None:
            raise RuntimeError('set_affine() needs a controller that has been set up')
        self.prob.set_affine(d)

    def affine(self):
        """The affine term in force [B, rows, nx] (rows: 1 or Np), or None."""
        return self.prob.affine()

    def update(self, x, u=None, xref=None, solve=True, d=None):
        if d is not None:
            self.set_affine(d)
        self.x0_rh = x
        if u is not None:
            self.uminus1_rh = u
        if xref is not None:
            self.xref = xref
        self.prob.update(self.x0_rh, self.uminus1_rh, xref)
        self._um1_on_device = True
        if solve:
            self.solve()

    def solve(self):
        self.prob.solve_async()
        self.solve_count += 1
        self._u_last = None

    def step(self, x, u=None, xref=None, out=None, d=None):
        """``u = K(x, u_{-1})``: ``update(x, u, xref)`` followed by ``output()`` in one library call
        (MPCController.__controller_function__, mpc.py:377-384).  ``out``: an array or torch device tensor [B,nu] to write the inputs into.
        ``d``: a new affine term first (``set_affine``); None leaves the one in force."""
        if d is not None:
            self.set_affine(d)
        self.x0_rh = x
        if u is not None:
            self.uminus1_rh = u
        if xref is not None:
            self.xref = xref
        if u is None and not self._um1_on_device:
            u = self.uminus1_rh                   # update(x, u=None) uses the input of the last output() (mpc.py:330,357-359)
        uMPC = self.prob.mpc_step(x, u, xref, out=out)
        self.solve_count += 1
        self.uminus1_rh = uMPC
        self._um1_on_device = True                # mpcqp_mpc_step stored it as the next u_{-1}
        self._u_last = None
        return uMPC

    def run(self, nsteps, w=None, Ap=None, Bp=None, xref_traj=None, estimator=None, model_traj=None, L_traj=None, d_traj=None, d_hold=1):
        """``nsteps`` closed-loop steps on the device, equivalent to
        ``for k in range(nsteps): u = K.output(); x = Ap @ x + Bp @ u + w[k]; K.update(x, u, xref_traj[k])``
        (the loop of examples/example_point_mass.py:88-101 with a linear plant; default plant = (Ad, Bd)), or, with
        ``estimator = BatchLinearStateEstimator`` (pympc_amd.kalman), to the output-feedback loop of
        examples/example_inverted_pendulum_kalman.py:135-174 -- the estimator object supplies C, L, the measurement noise
        ``estimator.v`` [nsteps,B,ny] (optional) and the true plant state ``estimator.x_true`` [B,nx], advanced in place.
        ``model_traj = (Ad [nmodels,B,nx,nx] or None, Bd [nmodels,B,nx,nu] or None, hold)``: a schedule of models -- entry ``k // hold`` replaces
        Ad / Bd at the start of step k (mpcqp_mpc_loop_tv: ``update_model`` between closed-loop launches, no host round trip); the controller is
        left with the last entry used.  With an estimator too (mpcqp_mpc_loop_tv_est, include_ext2/mpcqp_rollout_tv_est.h): the estimator steps
        under the entry in force, and ``L_traj`` [nentries,B,nx,ny] schedules its gain the same way (entry ``k // hold`` at step k; None: the
        estimator's own ``L`` throughout); the estimator object is left with the last estimate and, where scheduled, the last gain.
        ``d_traj`` [nentries,B,nx] or [nentries,B,Np,nx]: a schedule of affine terms (mpcqp_mpc_loop_affine) -- the solve after step k uses entry
        ``k // d_hold``, the indexing of ``model_traj`` and, at ``d_hold = 1``, of ``xref_traj[k]``; the plant does not get the offset (put it into
        ``w``); the controller is left with the last entry used.  Without it a term set with ``set_affine`` stays in force over the run.  Not
        with an estimator.
        Returns ``dict(x=[nsteps+1,B,nx], u=[nsteps,B,nu], status=[nsteps,B] (OSQP status values), iter=[nsteps,B])``
        plus ``xhat`` and ``y`` with an estimator."""
        if d_traj is not None and estimator is not None:
            raise NotImplementedError('run: output feedback under a schedule of affine terms is not implemented (include_ext4/mpcqp_affine.h)')
        if L_traj is not None and (estimator is None or model_traj is None):
            raise ValueError('run: L_traj schedules the gain of an estimator beside a model_traj: give both')
        if estimator is not None and model_traj is not None:
            out = self.prob.mpc_run_tv_est(nsteps, model_traj, _est_dict(estimator), L_traj=L_traj, w=w, Ap=Ap, Bp=Bp, xref_traj=xref_traj)
            self.solve_count += int(nsteps)               # (a library without the call has raised: the controller is not moved on)
            self._after_schedule(nsteps, model_traj, estimator, L_traj)
            return self._after_loop(out, xref_traj, estimator)
        self.solve_count += int(nsteps)
        out = self.prob.mpc_run(nsteps, w=w, Ap=Ap, Bp=Bp, xref_traj=xref_traj, estimator=_est_dict(estimator), model_traj=model_traj,
                                d_traj=d_traj, d_hold=d_hold)
        if model_traj is not None:
            self._after_schedule(nsteps, model_traj)
        return self._after_loop(out, xref_traj, estimator)

    def _after_schedule(self, nsteps, model_traj, estimator=None, L_traj=None):
        """The controller's Ad, Bd after a loop under a schedule: the last entry used.  With an estimator: its model is that entry too, and its
        gain the last entry of ``L_traj`` where there is one."""
        last = (int(nsteps) - 1) // int(model_traj[2])
        host = lambda a: np.array(a[last].detach().cpu() if hasattr(a, 'data_ptr') else a[last], dtype=float).reshape((self.B,) + tuple(a.shape[-2:]))
        if model_traj[0] is not None:
            self.Ad = host(model_traj[0])
        if model_traj[1] is not None:
            self.Bd = host(model_traj[1])
        if estimator is not None:
            if model_traj[0] is not None:
                estimator.A = self.Ad.copy()
            if model_traj[1] is not None:
                estimator.Bm = self.Bd.copy()
            if L_traj is not None:
                estimator.L = host(L_traj)

    def _after_loop(self, out, xref_traj, estimator=None, count=0):
        """The controller's books after a device loop of any kind, and its result dict: the controller stands at the last state (with an
        estimator: at the last estimate, which the estimator object gets too), the last reference and the last input, which is on the
        device as u_{-1}.  ``count``: steps to add to ``solve_count`` now (a rollout counts them once it has succeeded, ``run`` before the call)."""
        self.solve_count += count
        xt, ut, st, it = out[:4]
        res = dict(x=xt, u=ut, status=st, iter=it)
        if estimator is not None:
            res['xhat'], res['y'] = out[4], out[5]
            self.x0_rh = out[4][-1].copy()
            estimator.x = out[4][-1].copy()
        else:
            self.x0_rh = xt[-1].copy()
        if xref_traj is not None:
            self.xref = np.asarray(xref_traj)[-1].reshape(self.B, -1)
        self.uminus1_rh = ut[-1].copy()
        self._um1_on_device = True
        self._u_last = None
        return res

    def _rollout(self, nsteps, w, Ap, Bp, xref_traj, **form):
        """The taped loop of every form: the ``prob.rollout*`` that takes the options of ``form`` -- ``model_traj``, ``estimator``, ``L_traj``
        as the public method has them: which are there says which loop, so that the loop refuses one that is None -- then the controller's books.
        ``d_hold`` among them: the loop with an affine term, ``prob.rollout_affine``, whose ``model_traj`` and ``d_traj`` may both be None."""
        model_traj, estimator = form.get('model_traj'), form.get('estimator')
        if 'estimator' in form:
            form['estimator'] = _est_dict(estimator)
        roll = getattr(self.prob, 'rollout_affine' if 'd_hold' in form else
                       'rollout' + ('_tv' if 'model_traj' in form else '') + ('_est' if 'estimator' in form else ''))
        out = roll(nsteps, w=w, Ap=Ap, Bp=Bp, xref_traj=xref_traj, **form)
        if model_traj is not None:
            self._after_schedule(nsteps, model_traj, estimator, form.get('L_traj'))
        return self._after_loop(out, xref_traj, estimator, count=int(nsteps))

    def rollout(self, nsteps, w=None, Ap=None, Bp=None, xref_traj=None):
        """``run`` that keeps a tape (mpcqp_rollout, include/mpcqp_rollout.h): the same loop, the same dict, one closed-loop launch per
        step -- and afterwards ``rollout_adjoint`` differentiates a loss on the whole trajectory in one reverse sweep on the device.  No
        estimator and no model schedule in a taped rollout."""
        return self._rollout(nsteps, w, Ap, Bp, xref_traj)

    def rollout_tv(self, nsteps, model_traj, w=None, Ap=None, Bp=None, xref_traj=None):
        """``run(model_traj=)`` that keeps a tape (mpcqp_rollout_tv, include_ext/mpcqp_rollout_tv.h): the same loop under the same schedule
        ``model_traj = (Ad [nmodels,B,nx,nx] or None, Bd [nmodels,B,nx,nu] or None, hold)``, the same dict, the controller left with the last
        entry used -- and a tape that remembers every model it was made under, so that ``rollout_adjoint`` can differentiate a loss on the
        trajectory with respect to each schedule entry ('Ad_traj', 'Bd_traj', 'Ap_traj', 'Bp_traj') beside everything else."""
        return self._rollout(nsteps, w, Ap, Bp, xref_traj, model_traj=model_traj)

    def rollout_tv_est(self, nsteps, model_traj, estimator, L_traj=None, w=None, Ap=None, Bp=None, xref_traj=None):
        """``run(estimator=, model_traj=, L_traj=)`` that keeps a tape (mpcqp_rollout_tv_est, include_ext2/mpcqp_rollout_tv_est.h): the same
        output-feedback loop under the same schedule of models and, optionally, gains, the same dict, the controller left with the last entry
        used, the estimator object with the last estimate and, where scheduled, the last gain -- and a tape from which ``rollout_adjoint``
        differentiates a loss on states, estimates, inputs and measurements with respect to every schedule entry through its three paths:
        its solves ('Ad_traj', 'Bd_traj'), the plant ('Ap_traj', 'Bp_traj') and the estimator ('Ae_traj', 'Be_traj'), and to every gain
        entry ('L_traj')."""
        return self._rollout(nsteps, w, Ap, Bp, xref_traj, model_traj=model_traj, estimator=estimator, L_traj=L_traj)

    def rollout_affine(self, nsteps, d_traj=None, d_hold=1, model_traj=None, w=None, Ap=None, Bp=None, xref_traj=None):
        """``run(d_traj=, d_hold=, model_traj=)`` that keeps a tape (mpcqp_rollout_affine, include_ext5/mpcqp_rollout_affine.h): the same loop with
        the same indexing -- the solve after step k uses entry ``k // d_hold`` of ``d_traj`` [nent,B,nx] or [nent,B,Np,nx] (numpy or a torch device
        tensor) -- the same dict, the controller left with the last entry used; ``d_traj=None``: the term set with ``set_affine`` throughout (there
        must be one).  The tape remembers every term, so that ``rollout_adjoint`` can differentiate a loss on the trajectory with respect to the
        term the call began under ('d0') and every schedule entry ('d_traj') beside everything else.  The plant does not get the offset.  No
        estimator."""
        return self._rollout(nsteps, w, Ap, Bp, xref_traj, d_traj=d_traj, d_hold=d_hold, model_traj=model_traj)

    def rollout_est(self, nsteps, estimator, w=None, Ap=None, Bp=None, xref_traj=None):
        """``run(estimator=...)`` that keeps a tape (mpcqp_rollout_est, include/mpcqp_rollout_est.h): the output-feedback loop with a
        ``BatchLinearStateEstimator`` -- the same dict (``x, u, status, iter, xhat, y``), ``estimator.x_true`` advanced in place -- and afterwards
        ``rollout_adjoint`` differentiates a loss on states, estimates, inputs and measurements through controller, plant and estimator."""
        return self._rollout(nsteps, w, Ap, Bp, xref_traj, estimator=estimator)

    def rollout_adjoint(self, g_x=None, g_u=None, want=('lam', 'uminus1', 'uref', 'xref'), batch_sum=False, no_reuse=False, g_xhat=None, g_y=None):
        """Push a loss on the trajectory of the last ``rollout`` back through the closed loop (mpcqp_rollout_adjoint): ``g_x`` [K+1,B,nx] =
        dL/dx_k, ``g_u`` [K,B,nu] = dL/du_k.  Returns the gradients named in ``want`` -- 'lam' [K+1,B,nx] (lam[0] = dL/dx0, lam[k+1] =
        dL/dw[k]), 'uminus1', 'uref' [B,nu], 'xref' [K,B,rows*nx], 'Ap' [B,nx,nx], 'Bp' [B,nx,nu] (the plant path alone: with the
        controller's own model as the plant, add them to 'Ad', 'Bd'), and 'Ad', 'Bd', 'Qx', 'QxN', 'Qu', 'QDu', 'eps_feas' summed over the
        steps (``batch_sum``: and over the batch), and likewise the bound gradients 'xmin', 'xmax' [B,nx], 'umin', 'umax', 'Dumin', 'Dumax'
        [B,nu] (mpcqp_rollout_adjoint_bounds: the bounds are constant over the tape) -- plus ``n_weak`` [K,B], ``status`` [K,B] per step and ``n_factor`` [B], the
        factorizations the sweep made.  numpy in, numpy out; torch device tensors in, device tensors out.  After ``rollout_est``: ``g_xhat``
        [K+1,B,nx] = dL/dxhat_k and ``g_y`` [K,B,ny] = dL/dy_k seed the sweep too, and ``want`` may name 'eta' [K+1,B,nx] (eta[0] = dL/dxhat_0),
        'C' [B,ny,nx], 'L' [B,nx,ny], 'v' [K,B,ny] and 'Ae' [B,nx,nx], 'Be' [B,nx,nu], the estimator path alone (add them to 'Ad', 'Bd').
        After ``rollout_tv``: ``want`` may name 'Ad_traj' [nseg,B,nx,nx], 'Bd_traj' [nseg,B,nx,nu] (entry e: through the solves made under
        schedule entry e) and 'Ap_traj', 'Bp_traj' (entry e: through the plant while entry e was in force; where the plant followed the
        schedule, add them); 'Ad', 'Bd' are then the share of the model the rollout began with.
        After ``rollout_tv_est``: all of both, and 'Ae_traj' [nseg,B,nx,nx], 'Be_traj' [nseg,B,nx,nu], 'L_traj' [nseg,B,nx,ny] (entry e: through
        the estimator while entry e was in force); 'Ae', 'Be', 'L' are their sums over the entries.
        After ``rollout_affine`` (mpcqp_rollout_adjoint_affine): everything above that its tape allows (the ``_traj`` names where it was given a
        ``model_traj``), and 'd0' [B,rows*nx] -- through the solves made under the term the call began with: entry 0's, and every entry's where
        no ``d_traj`` was given -- and 'd_traj' [nent,B,rows*nx], entry e: through the solves made under schedule entry e (an entry no solve
        used: zeros); ``batch_sum`` sums both over the instances ([1,..] and [nent,1,..]).  On any other tape the two names raise."""
        res = self.prob.rollout_adjoint(g_x=g_x, g_u=g_u, want=want, batch_sum=batch_sum, no_reuse=no_reuse, g_xhat=g_xhat, g_y=g_y)
        _, n_weak, status, n_factor = self.prob.rollout_info()
        res.update(n_weak=n_weak, status=status, n_factor=n_factor)
        return res

    def gains(self, like=None):
        """Local gains of the constrained control law of every instance at its last solve (mpcqp_gains, include/mpcqp_adjoint.h):
        ``dict(K_x0 [B,nu,nx], K_um1 [B,nu,nu], K_xref [B,nu,rows*nx], K_uref [B,nu,nu], n_weak [B], status [B])`` -- the Jacobians of u_0
        for the active set the iterate implies; the key names follow ``pympc_amd.unconstrained``.  ``like``: a torch device tensor to get
        device tensors back.  ``n_weak > 0``: a kink of the law, one-sided gains; ``status`` 1 computed, 0 not solved (zeros), -1 broken
        factorization (zeros).  With an affine term in force (``set_affine``) also ``K_d`` [B,nu,rows*nx] = d u_0 / d d, the feed-forward gain of the
        term in the shape it was set in (mpcqp_gains_affine: the same factorization and seeds; row j is ``adjoint(g_u0=e_j, want=('d',))['d']``);
        without a term the dict has no such key."""
        g = self.prob.gains(like=like)
        _, n_weak, status = self.prob.adjoint_info()
        res = dict(K_x0=g['x0'], K_um1=g['uminus1'], K_xref=g['xref'], K_uref=g['uref'], n_weak=n_weak, status=status)
        if 'd' in g:
            res['K_d'] = g['d']
        return res

    def adjoint(self, g_u0=None, g_w=None, want=('x0', 'uminus1', 'xref', 'uref'), batch_sum=False):
        """Vector-Jacobian products of the last solve (mpcqp_adjoint): for ``g_u0`` [B,nu] = dL/du_0 and / or ``g_w`` [B,n] = dL/dw returns
        ``dict(x0 [B,nx], uminus1 [B,nu], xref [B,rows*nx], uref [B,nu], n_weak [B], status [B])`` = dL/d(x0, u_{-1}, xref, uref).  ``want`` may
        also name the model gradients 'Ad' [B,nx,nx], 'Bd' [B,nx,nu], 'Qx', 'QxN' [B,nx,nx], 'Qu', 'QDu' [B,nu,nu], 'eps_feas' [B]
        (mpcqp_adjoint_model; ``batch_sum``: summed over the batch, leading dimension 1 -- see ``BatchProblem.adjoint``) and the bound
        gradients 'xmin', 'xmax' [B,nx], 'umin', 'umax', 'Dumin', 'Dumax' [B,nu] (mpcqp_adjoint_bounds; ``batch_sum`` likewise) and 'd'
        [B,rows*nx], the gradient of the affine term in force (mpcqp_adjoint_affine).  numpy in,
        numpy out; torch device tensors in, device tensors out."""
        res = self.prob.adjoint(g_w=g_w, g_u0=g_u0, want=want, batch_sum=batch_sum)
        _, n_weak, status = self.prob.adjoint_info()
        res.update(n_weak=n_weak, status=status)
        return res

    def status(self):
        """Per-instance OSQP status strings of the last solve."""
        infos = self.prob.infos()
        self._infos = infos
        return [self.prob.status_string(i.status) for i in infos]

    def output(self, return_status=False, return_x_seq=False, return_u_seq=False, return_eps_seq=False,
               return_obj_val=False):
        nx, nu, Np, Nc = self.nx, self.nu, self.Np, self.Nc
        want_seq = return_x_seq or return_u_seq or return_eps_seq
        info = {}
        if want_seq:
            x, _, infos = self.prob.solution(want_y=False)
            u0 = x[:, (Np + 1) * nx:(Np + 1) * nx + nu].copy()
        else:
            u0 = self.prob.u0()
            infos = self.prob.infos()
        solved = np.array([i.status == 1 for i in infos])
        uMPC = np.where(solved[:, None], u0, self.u_failure)
        if return_x_seq:
            info['x_seq'] = x[:, :(Np + 1) * nx].reshape(self.B, Np + 1, nx)
        if return_u_seq:
            info['u_seq'] = x[:, (Np + 1) * nx:(Np + 1) * nx + Nc * nu].reshape(self.B, Nc, nu)
        if return_eps_seq:
            o = (Np + 1) * nx + Nc * nu
            info['eps_seq'] = x[:, o:o + (Np + 1) * nx].reshape(self.B, -1, nx)          # (empty without slack variables)
        if return_status:
            info['status'] = [self.prob.status_string(i.status) for i in infos]
            info['iter'] = np.array([i.iter for i in infos])
        if return_obj_val:
            info['obj_val'] = np.array([i.obj_val for i in infos])
        self.uminus1_rh = uMPC
        self._um1_on_device = False
        return uMPC if len(info) == 0 else (uMPC, info)
