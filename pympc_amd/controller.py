"""Drop-in replacement for ``pyMPC.mpc.MPCController`` (reference: pyMPC/mpc.py:27-616).

Same constructor signature, defaults, error messages, public attributes and
``setup / update / solve / output / __controller_function__`` semantics.  The difference is
what sits behind ``self.prob``: instead of ``osqp.OSQP()`` (mpc.py:241) it is a
``pympc_amd.solver.DeviceProblem`` -- a ctypes handle onto ``libmpcqp_hip.so``, the
hand-written HIP implementation of the QP build and of the OSQP-style ADMM loop for gfx950.

The hidden switch ``SOFT_ON = False`` (mpc.py:237: hard state box, no slack variables) is honoured on the device.
There is NO CPU fallback: if the HIP library or a GPU is missing, ``setup()`` raises.
(Tests that exercise only the host logic inject their own ``prob`` object.)
"""
import warnings

import numpy as np
import scipy.sparse as sparse

from . import qp_build

# (attribute, expected length attribute, ravel?, message) -- mirrors the checks of mpc.py:107-223
_ERR = {
    'x0': "x0 should be an array of dimension (nx,)!",
    'xref': "xref should be either a vector of shape (nx,) or a matrix of shape (Np+1, nx)!",
    'uref': "uref should be a vector of shape (nu,)!",
    'uminus1': "uminus1 should be a vector of shape (nu,)!",
    'Qx': "Qx should be a matrix of shape (nx, nx)!",
    'QxN': "QxN should be a square matrix of shape (nx, nx)!",
    'Qu': "Qu should be a square matrix of shape (nu, nu)!",
    'QDu': "QDu should be a square matrix of shape (nu, nu)!",
    'xmin': "xmin should be a vector of shape (nx,)!",
    'xmax': "xmax should be a vector of shape (nx,)!",
    'umin': "umin should be a vector of shape (nu,)!",
    'umax': "umax should be a vector of shape (nu,)!",
    'Dumin': "Dumin should be a vector of shape (nu,)!",
    'Dumax': "Dumax should be a vector of shape (nu,)!",
}


def _vector_like(v):
    """The reference's ``__is_vector__`` (mpc.py:8-17): 1-D, or 2-D with a leading 1 (or an
    empty second axis); anything else -- including (k, 1) columns -- is rejected."""
    if v.ndim == 1:
        return True
    return v.ndim == 2 and (v.shape[0] == 1 or v.shape[1] == 0)


def _matrix_like(M):
    return M.ndim == 2


class MPCController:
    """Linear constrained MPC controller; see the reference class docstring (mpc.py:28-74)
    for the meaning of every argument.  All arguments, defaults and failure modes match."""

    def __init__(self, Ad, Bd, Np=20, Nc=None,
                 x0=None, xref=None, uref=None, uminus1=None,
                 Qx=None, QxN=None, Qu=None, QDu=None,
                 xmin=None, xmax=None, umin=None, umax=None, Dumin=None, Dumax=None,
                 eps_feas=1e6, eps_rel=1e-3, eps_abs=1e-3):
        if not (_matrix_like(Ad) and Ad.shape[0] == Ad.shape[1]):
            raise ValueError("Ad should be a square matrix of dimension (nx,nx)!")
        self.Ad = Ad
        self.nx = nx = Ad.shape[0]
        if not (_matrix_like(Bd) and Bd.shape[0] == nx):
            raise ValueError("Bd should be a matrix of dimension (nx, nu)!")
        self.Bd = Bd
        self.nu = nu = Bd.shape[1]
        if not Np > 1:
            raise ValueError("Np should be > 1!")
        self.Np = Np
        if Nc is not None and not Nc <= Np:
            raise ValueError("Nc should be <= Np!")
        self.Nc = Np if Nc is None else Nc

        def vec(name, val, size, default, ravel):
            if val is None:
                return default()
            if not (_vector_like(val) and val.size == size):
                raise ValueError(_ERR[name])
            return val.ravel() if ravel else val

        def mat(name, val, size, default):
            if val is None:
                return default()
            if not (_matrix_like(val) and val.shape[0] == size and val.shape[1] == size):
                raise ValueError(_ERR[name])
            return val

        self.x0 = vec('x0', x0, nx, lambda: np.zeros(nx), True)
        if xref is None:
            self.xref = np.zeros(nx)
        elif _vector_like(xref) and xref.size == nx:
            self.xref = xref.ravel()
        elif _matrix_like(xref) and xref.shape[1] == nx and xref.shape[0] >= Np:
            self.xref = xref
        else:
            raise ValueError(_ERR['xref'])
        self.uref = vec('uref', uref, nu, lambda: np.zeros(nu), True)
        # NB: default uminus1 ALIASES uref, like mpc.py:141
        self.uminus1 = vec('uminus1', uminus1, nu, lambda: self.uref, False)

        self.Qx = mat('Qx', Qx, nx, lambda: np.zeros((nx, nx)))
        if QxN is None:
            self.QxN = self.Qx
        else:
            # the reference reads Qx.shape[1] in this check (mpc.py:153); with Qx=None that is an
            # AttributeError there as well
            if not (_matrix_like(QxN) and QxN.shape[0] == nx and Qx.shape[1] == nx):
                raise ValueError(_ERR['QxN'])
            self.QxN = QxN
        self.Qu = mat('Qu', Qu, nu, lambda: np.zeros((nu, nu)))
        self.QDu = mat('QDu', QDu, nu, lambda: np.zeros((nu, nu)))

        inf = np.inf
        self.xmin = vec('xmin', xmin, nx, lambda: -np.ones(nx) * inf, True)
        self.xmax = vec('xmax', xmax, nx, lambda: np.ones(nx) * inf, False)
        self.umin = vec('umin', umin, nu, lambda: -np.ones(nu) * inf, False)
        self.umax = vec('umax', umax, nu, lambda: np.ones(nu) * inf, False)
        self.Dumin = vec('Dumin', Dumin, nu, lambda: -np.ones(nu) * inf, False)
        self.Dumax = vec('Dumax', Dumax, nu, lambda: np.ones(nu) * inf, False)

        self.eps_feas = eps_feas
        self.Qeps = eps_feas * sparse.eye(nx)
        self.eps_rel = eps_rel
        self.eps_abs = eps_abs
        self.u_failure = self.uref      # returned by output() when the solve failed

        # hidden debug switches of mpc.py:233-238
        self.raise_error = False
        self.JX_ON = True
        self.JU_ON = True
        self.JDU_ON = True
        self.SOFT_ON = True
        self.COMPUTE_J_CNST = False

        # Solver instance.  Created lazily in setup() so that constructing a controller never
        # touches the GPU; tests may assign their own object here before setup().
        self.prob = None
        # extra solver settings forwarded to the device problem (additive surface)
        self.solver_settings = {}

        self.res = None
        self.P = None
        self._q = self._l = self._u = self._J_CNST = None
        self._stale = False           # q, l, u, J_CNST not yet refreshed after the last update() (device solver only)
        self.A = None
        self.P_X = None
        self.x0_rh = None
        self.uminus1_rh = None
        self.d = None                 # the affine term of the prediction model in force, [nx] or [Np, nx] (set_affine / update(d=)); None: none

    # ------------------------------------------------------------------------------------
    def _model_data(self):
        """Raw controller data handed to the device, which builds P,q,A,l,u itself."""
        d = lambda M: M.toarray() if sparse.issparse(M) else np.asarray(M, dtype=float)
        return dict(
            nx=self.nx, nu=self.nu, Np=self.Np, Nc=self.Nc,
            Ad=d(self.Ad), Bd=d(self.Bd),
            Qx=d(self.Qx) if self.JX_ON else np.zeros((self.nx, self.nx)),
            QxN=d(self.QxN) if self.JX_ON else np.zeros((self.nx, self.nx)),
            Qu=d(self.Qu) if self.JU_ON else np.zeros((self.nu, self.nu)),
            QDu=d(self.QDu) if self.JDU_ON else np.zeros((self.nu, self.nu)),
            xmin=self.xmin, xmax=self.xmax, umin=self.umin, umax=self.umax,
            Dumin=self.Dumin, Dumax=self.Dumax, eps_feas=float(self.eps_feas),
            x0=np.asarray(self.x0_rh, dtype=float), uminus1=np.asarray(self.uminus1_rh, dtype=float),
            xref=np.asarray(self.xref, dtype=float), uref=np.asarray(self.uref, dtype=float),
            SOFT_ON=bool(self.SOFT_ON),
        )

    def _step_data(self):
        return dict(x0=np.asarray(self.x0_rh, dtype=float),
                    uminus1=np.asarray(self.uminus1_rh, dtype=float),
                    xref=np.asarray(self.xref, dtype=float))

    def setup(self, solve=True):
        """Build the QP and set the solver up (mpc.py:254-269); optionally solve it."""
        self.x0_rh = np.copy(self.x0)
        self.uminus1_rh = np.copy(self.uminus1)
        self.d = None                         # (a new setup starts without an affine term)
        self._compute_QP_matrices_()
        if self.prob is None:
            from .solver import DeviceProblem   # raises loudly without the HIP library / a GPU
            self.prob = DeviceProblem()
        # the reference passes eps_abs=self.eps_rel, eps_rel=self.eps_abs (swapped, mpc.py:266)
        self.prob.setup(self.P, self.q, self.A, self.l, self.u, warm_start=True, verbose=False,
                        eps_abs=self.eps_rel, eps_rel=self.eps_abs,
                        mpc=self._model_data(), **self.solver_settings)
        if solve:
            self.solve()

    def output(self, return_x_seq=False, return_u_seq=False, return_eps_seq=False,
               return_status=False, return_obj_val=False):
        """First optimal input (or ``u_failure``) and optional info dict (mpc.py:271-336)."""
        Np, Nc, nx, nu = self.Np, self.Nc, self.nx, self.nu
        ou = (Np + 1) * nx
        oe = ou + Nc * nu
        if self.res.info.status == 'solved':
            uMPC = self.res.x[ou:ou + nu]
        else:
            uMPC = self.u_failure
        info = {}
        if return_x_seq:
            info['x_seq'] = self.res.x[0:ou].reshape(-1, nx)
        if return_u_seq:
            info['u_seq'] = self.res.x[ou:oe].reshape(-1, nu)
        if return_eps_seq:
            info['eps_seq'] = self.res.x[oe:oe + ou].reshape(-1, nx)
        if return_status:
            info['status'] = self.res.info.status
        if return_obj_val:
            info['obj_val'] = self.res.info.obj_val + self.J_CNST
        self.uminus1_rh = uMPC
        return uMPC if len(info) == 0 else (uMPC, info)

    def set_affine(self, d):
        """The affine term of the prediction model, x_{k+1} = Ad x_k + Bd u_k + d_k (mpcqp_set_affine, include_ext4/mpcqp_affine.h): ``d`` [nx] -- the
        offset c = f(xbar, ubar) - Ad xbar - Bd ubar of a linearisation away from an equilibrium, used at every stage -- or [Np, nx], row k for the
        step k -> k+1 (a previewed disturbance); ``None`` clears it.  It stays in force across update(), update_model() and solve() until it
        is replaced or cleared; setup() clears it.  The dynamics rows of ``l``, ``u`` become -d; no factorization is made.  The next solve uses
        it (this call does not solve).  An addition to the reference's class; it needs the device solver behind ``prob``."""
        if not hasattr(self.prob, 'set_affine'):
            raise NotImplementedError('set_affine() needs the device solver behind prob (pympc_amd.solver.DeviceProblem)')
        nx, Np = self.nx, self.Np
        if d is not None:
            d = np.array(d, dtype=float)
            if d.shape not in ((nx,), (Np, nx)):
                raise ValueError('d should be a vector of dimension nx or a matrix of dimension (Np, nx)!')
        self.prob.set_affine(d)
        self.d = d
        if self._l is not None:                   # (the public l, u: rows (k+1) nx .. of the dynamics block carry 0.0 - d_k)
            rows = np.zeros(Np * nx) if d is None else 0.0 - np.broadcast_to(d, (Np, nx)).ravel()
            self._l[nx:(Np + 1) * nx] = rows
            self._u[nx:(Np + 1) * nx] = rows

    def update(self, x, u=None, xref=None, solve=True, d=None):
        """New measurement (and optionally u_{-1}, xref): refresh q,l,u and re-solve (mpc.py:338-364).  ``d``: a new affine term of the
        prediction model for this and the following solves (``set_affine``); None leaves the one in force as it is."""
        if d is not None:
            self.set_affine(d)
        self.x0_rh = x
        if u is not None:
            self.uminus1_rh = u
        if xref is not None:
            self.xref = xref
        self._update_QP_matrices_()
        if solve:
            self.solve()
        elif hasattr(self.prob, 'flush'):
            self.prob.flush()                 # (the device solver sends the step data with the solve; without one, now)

    def update_model(self, Ad=None, Bd=None, Qx=None, QxN=None, Qu=None, QDu=None,
                     xmin=None, xmax=None, umin=None, umax=None, Dumin=None, Dumax=None,
                     uref=None, eps_feas=None, solve=True):
        """New controller data for a controller that is in use -- a relinearised plant, scheduled weights or bounds; an addition to the
        reference's class, which can only be constructed again.  Every argument left at None keeps its value (QxN included: it does not
        follow a new Qx).  The arguments are checked like the constructor's, with its messages; dimensions cannot change.  The public
        attributes and P, q, A, l, u are rebuilt for the current x0 / u_{-1} / xref, and the solver takes the new problem WITHOUT losing
        its iterate: ``prob.update_model`` where the solver has it (the device re-equilibrates, refactors and keeps x, y), otherwise a fresh
        ``type(prob)()`` set up with the new matrices and warm-started from ``res.x, res.y``.  Before ``setup()`` only the attributes change."""
        nx, nu = self.nx, self.nu
        new = {}
        if Ad is not None:
            if not (_matrix_like(Ad) and Ad.shape[0] == Ad.shape[1] and Ad.shape[0] == nx):
                raise ValueError("Ad should be a square matrix of dimension (nx,nx)!")
            new['Ad'] = Ad
        if Bd is not None:
            if not (_matrix_like(Bd) and Bd.shape[0] == nx and Bd.shape[1] == nu):
                raise ValueError("Bd should be a matrix of dimension (nx, nu)!")
            new['Bd'] = Bd
        for name, val, size in (('Qx', Qx, nx), ('Qu', Qu, nu), ('QDu', QDu, nu)):
            if val is not None:
                if not (_matrix_like(val) and val.shape[0] == size and val.shape[1] == size):
                    raise ValueError(_ERR[name])
                new[name] = val
        if QxN is not None:
            if not (_matrix_like(QxN) and QxN.shape[0] == nx and QxN.shape[1] == nx):
                raise ValueError(_ERR['QxN'])
            new['QxN'] = QxN
        for name, val, size, ravel in (('xmin', xmin, nx, True), ('xmax', xmax, nx, False), ('umin', umin, nu, False), ('umax', umax, nu, False),
                                       ('Dumin', Dumin, nu, False), ('Dumax', Dumax, nu, False), ('uref', uref, nu, True)):
            if val is not None:
                if not (_vector_like(val) and val.size == size):
                    raise ValueError(_ERR[name])
                new[name] = val.ravel() if ravel else val
        if eps_feas is not None:
            new['eps_feas'] = eps_feas
        if not new:
            raise ValueError("update_model needs at least one of Ad, Bd, Qx, QxN, Qu, QDu, xmin, xmax, umin, umax, Dumin, Dumax, uref, eps_feas!")
        for k, v in new.items():
            setattr(self, k, v)
        if 'eps_feas' in new:
            self.Qeps = eps_feas * sparse.eye(nx)
        if 'uref' in new:
            self.u_failure = self.uref
        if self.prob is None or self.P is None:          # not set up yet: setup() builds from the attributes
            return
        self._stale = False
        self._compute_QP_matrices_()                     # (from x0, uminus1 like setup(); then for the step data in force, like update())
        self.q, self.J_CNST = qp_build.refresh_vectors(self)
        if hasattr(self.prob, 'update_model') and getattr(self.prob, 'supports_update_model', True):
            md = self._model_data()
            # (the weights as the debug switches JX_ON / JU_ON / JDU_ON leave them; the step data as this call sees it: output() may have moved u_{-1} on)
            self.prob.update(mpc_step=(np.array(md['x0'], dtype=float).reshape(1, -1), np.array(md['uminus1'], dtype=float).reshape(1, -1),
                                       np.array(md['xref'], dtype=float).reshape(1, -1)))
            self.prob.update_model(**{k: md[k] for k in new})
        else:
            prob = type(self.prob)()
            prob.setup(self.P, self.q, self.A, self.l, self.u, warm_start=True, verbose=False,
                       eps_abs=self.eps_rel, eps_rel=self.eps_abs, mpc=self._model_data(), **self.solver_settings)
            if self.res is not None:
                prob.warm_start(x=self.res.x, y=self.res.y)
            self.prob = prob
        if solve:
            self.solve()

    def solve(self):
        """Warm-started solve (mpc.py:366-375)."""
        self.res = self.prob.solve()
        if self.res.info.status != 'solved':
            warnings.warn('OSQP did not solve the problem!')
            if self.raise_error:
                raise ValueError('OSQP did not solve the problem!')

    def __controller_function__(self, x, u, xref=None):
        """u = K(x, u_{-1}) as a pure function (mpc.py:377-384)."""
        self.update(x, u, xref=xref, solve=True)
        return self.output()

    def unconstrained_gains(self, tol=1e-13):
        """Gain matrices of this controller's law without inequality constraints, U* = K_x0 x0 + K_xref xref + K_uref uref + K_um1 u_{-1}
        (test_scripts/alternative/unconstrained.py:170-183), computed on the device (pympc_amd/unconstrained.py: one KKT factorization, a
        few batched solves).  An addition to the reference's class; output() does not use it.  An affine term (``set_affine``) is ignored:
        these are the gains of the linear part of the law, the term only adds a constant to U*."""
        from .unconstrained import unconstrained_gains, GainSolver
        d = lambda M: np.asarray(M.toarray() if hasattr(M, 'toarray') else M, dtype=float)        # (scipy.sparse inputs are accepted like in the reference)
        gs = getattr(self, '_gain_solver', None)
        if gs is None or gs.tol != tol:
            gs = self._gain_solver = GainSolver(self.nx, self.nu, self.Np, self.Nc, tol=tol)      # (kept: a second call allocates nothing)
        return unconstrained_gains(d(self.Ad), d(self.Bd), self.Np, self.Nc, Qx=d(self.Qx), QxN=d(self.QxN), Qu=d(self.Qu), QDu=d(self.QDu), tol=tol, solver=gs)

    def gains(self):
        """Local gains of the CONSTRAINED control law at the last solve: ``dict(K_x0 [nu, nx], K_um1 [nu, nu], K_xref [nu, rows*nx],
        K_uref [nu, nu], n_weak, status)`` -- du_0/dx0, du_0/du_{-1}, du_0/dxref, du_0/duref of the active set the iterate implies
        (mpcqp_gains, include/mpcqp_adjoint.h: one factorization on the device, nu adjoint solves).  With no inequality active they are the
        first nu rows of ``unconstrained_gains()``.  ``n_weak > 0``: the state sits on a kink of the piecewise affine law and the gains
        are one-sided; ``status`` 1 computed, 0 the last solve did not end 'solved' (zeros).  Solve tightly, or with ``polish=True``, where
        the active set must be the true one.  An addition to the reference's class."""
        bp = getattr(self.prob, 'batch_problem', None)
        if bp is None or not hasattr(bp, 'gains'):
            raise NotImplementedError('gains() needs the device solver behind prob (pympc_amd.solver.DeviceProblem)')
        g = bp.gains()
        _, n_weak, status = bp.adjoint_info()
        return dict(K_x0=g['x0'][0], K_um1=g['uminus1'][0], K_xref=g['xref'][0], K_uref=g['uref'][0], n_weak=int(n_weak[0]), status=int(status[0]))

    def adjoint(self, g_u0=None, g_w=None, want=('x0', 'uminus1', 'xref', 'uref')):
        """Vector-Jacobian products of the last solve for the seed ``g_u0`` [nu] = dL/du_0 and / or ``g_w`` [n] = dL/dw (mpcqp_adjoint,
        mpcqp_adjoint_model): a dict with the gradients named in ``want`` -- 'x0', 'uminus1', 'xref', 'uref', 'q', 'l', 'u' and the model
        gradients 'Ad' [nx, nx], 'Bd' [nx, nu], 'Qx', 'QxN' [nx, nx], 'Qu', 'QDu' [nu, nu], 'eps_feas' (weights: with respect to a symmetric
        perturbation) and the bound gradients 'xmin', 'xmax' [nx], 'umin', 'umax', 'Dumin', 'Dumax' [nu] (mpcqp_adjoint_bounds) and 'd', the
        gradient of the affine term in the shape it was set in (mpcqp_adjoint_affine) -- plus
        ``n_weak`` and ``status`` as in ``gains()``.  A weight whose cost term this controller runs without (the
        switches JX_ON, JU_ON, JDU_ON) gets zero.  An addition to the reference's class."""
        bp = getattr(self.prob, 'batch_problem', None)
        if bp is None or not hasattr(bp, 'adjoint'):
            raise NotImplementedError('adjoint() needs the device solver behind prob (pympc_amd.solver.DeviceProblem)')
        one = lambda a: None if a is None else np.asarray(a, dtype=float).reshape(1, -1)
        res = bp.adjoint(g_w=one(g_w), g_u0=one(g_u0), want=want)
        _, n_weak, status = bp.adjoint_info()
        res = {k: v[0] for k, v in res.items()}
        if 'd' in res and self.d is not None:
            res['d'] = res['d'].reshape(self.d.shape)
        off = {'Qx': self.JX_ON, 'QxN': self.JX_ON, 'Qu': self.JU_ON, 'QDu': self.JDU_ON}
        for k, on in off.items():
            if k in res and not on:
                res[k] = np.zeros_like(res[k])
        res.update(n_weak=int(n_weak[0]), status=int(status[0]))
        return res

    # ------------------------------------------------------------------------------------
    # q, l, u, J_CNST are public attributes of the reference (mpc.py:598-606).  The device solver rebuilds them itself from
    # (x0, u_{-1}, xref), so after update() the host copies are refreshed only when somebody reads them.
    def _fresh(self):
        if self._stale:
            self._stale = False
            # the QP that was handed to the solver: built from the values update() saw, not from what x0_rh /
            # uminus1_rh / xref have become since (output() moves uminus1_rh on, callers may reuse their x array)
            live = self.x0_rh, self.uminus1_rh, self.xref
            self.x0_rh, self.uminus1_rh, self.xref = self._snap
            try:
                self._q, self._J_CNST = qp_build.refresh_vectors(self)
            finally:
                self.x0_rh, self.uminus1_rh, self.xref = live

    q = property(lambda self: (self._fresh(), self._q)[1], lambda self, v: setattr(self, '_q', v))
    l = property(lambda self: (self._fresh(), self._l)[1], lambda self, v: setattr(self, '_l', v))
    u = property(lambda self: (self._fresh(), self._u)[1], lambda self, v: setattr(self, '_u', v))
    J_CNST = property(lambda self: (self._fresh(), self._J_CNST)[1], lambda self, v: setattr(self, '_J_CNST', v))

    def _update_QP_matrices_(self):
        from .solver import DeviceProblem
        if isinstance(self.prob, DeviceProblem):
            self._stale = True                    # refreshed on first read, from a snapshot of this call's inputs
            self._snap = (np.array(self.x0_rh, dtype=float), np.array(self.uminus1_rh, dtype=float), np.array(self.xref, dtype=float))
            self.prob.update(mpc_step=self._snap)      # (the snapshot itself: private copies, float64, contiguous -- nothing to convert again on the way down)
        else:                                     # a solver that wants the vectors (the oracle in the tests)
            self._stale = False
            self.q, self.J_CNST = qp_build.refresh_vectors(self)
            self.prob.update(l=self.l, u=self.u, q=self.q, mpc_step=self._step_data())

    def _compute_QP_matrices_(self):
        self.P, self.q, self.A, self.l, self.u, self.P_X, self.J_CNST = qp_build.build_qp(self)
