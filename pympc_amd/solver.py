"""Python face of the HIP solver.

``BatchProblem``  -- a batch of independent MPC instances of equal dimensions living on one GPU
                     (thin, 1:1 wrapper over the C ABI of include/mpcqp.h).
``DeviceProblem`` -- the object ``MPCController`` keeps in ``self.prob`` where the reference keeps
                     ``osqp.OSQP()`` (pyMPC/mpc.py:241): ``setup / update / solve`` with the call
                     shapes of mpc.py:266, 454, 369, returning an osqp-like result object.

Arrays may be numpy ndarrays (host) or torch CUDA tensors (device-resident); both are passed as
raw pointers, PyTorch being used only as a device-memory container.
"""
import collections
import ctypes as C
import math

import numpy as np

from . import _lib

_SETTING_NAMES = [f[0] for f in _lib.Settings._fields_]
# accepted for call compatibility with osqp, without effect on this solver
_IGNORED_SETTINGS = ('verbose', 'linsys_solver', 'time_limit', 'scaled_termination', 'adaptive_rho_fraction')
# osqp's solution polishing (include/mpcqp_polish.h): applied with mpcqp_set_polish, any time after the handle exists
_POLISH_SETTINGS = ('polish', 'delta', 'polish_refine_iter')


# fixed when the handle is created / set up: mpcqp_update_settings keeps the handle's own values (include/mpcqp.h)
_FIXED_AT_CREATE = ('rho', 'sigma', 'scaling', 'soft_constraints', 'backend', 'tuning')

_STATUS_STRINGS = {}       # status code -> OSQP's string (filled from mpcqp_status_string on first use)

# the tape a handle holds: its steps, the rows of its references, the outputs of its estimator (0: state feedback), and None or
# (hold, nseg, the schedule gave Ad, the schedule gave Bd) of the model schedule it was made under, and None or (rows, hold, nslots) of the affine
# terms it was made under (rollout_affine; hold 0: one constant term, one slot)
_Tape = collections.namedtuple('_Tape', 'K rows ny sched aff', defaults=(None,))

# the extensions beside include/mpcqp.h: feature -> (is it in the loaded library, what BatchProblem._need says where it is not)
_FEATURES = dict(
    polish=(_lib.has_polish, 'no solution polishing (include/mpcqp_polish.h)'),
    adjoint=(_lib.has_adjoint, 'no adjoint derivatives (include/mpcqp_adjoint.h)'),
    adjoint_model=(_lib.has_adjoint_model, 'no model gradients (include/mpcqp_adjoint_model.h)'),
    adjoint_bounds=(_lib.has_adjoint_bounds, 'no bound gradients (include/mpcqp_adjoint_bounds.h)'),
    rollout=(_lib.has_rollout, 'no taped rollout (include/mpcqp_rollout.h)'),
    rollout_est=(_lib.has_rollout_est, 'no taped output-feedback rollout (include/mpcqp_rollout_est.h)'),
    rollout_tv=(_lib.has_rollout_tv, 'no taped rollout under a model schedule (include_ext/mpcqp_rollout_tv.h)'),
    rollout_tv_est=(_lib.has_rollout_tv_est, 'no output-feedback loop under a model schedule (include_ext2/mpcqp_rollout_tv_est.h)'),
    model_update=(_lib.has_model_update, 'no in-place model update (include/mpcqp_model.h)'),
    model_traj=(_lib.has_model_update, 'no model schedule for the device loop (include/mpcqp_model.h)'),
    affine=(_lib.has_affine, 'no affine term in the prediction model (include_ext4/mpcqp_affine.h)'),
    rollout_affine=(_lib.has_rollout_affine, 'no taped rollout with an affine term (include_ext5/mpcqp_rollout_affine.h)'))


def _ptr(a):
    if a is None:
        return None
    if hasattr(a, 'data_ptr'):             # torch tensor (device or host)
        return C.c_void_p(a.data_ptr())
    return C.c_void_p(a.ctypes.data)


def _prep_out(a, shape, name):
    """An array / tensor the library writes ``shape`` doubles into: it must be float64, C-contiguous and hold exactly that many (the C ABI
    carries no sizes); returned as it is."""
    size = int(np.prod(shape))
    if hasattr(a, 'data_ptr'):
        import torch
        ok = a.dtype == torch.float64 and a.is_contiguous() and a.numel() == size
    else:
        ok = type(a) is np.ndarray and a.dtype == np.float64 and a.flags.c_contiguous and a.flags.writeable and a.size == size
    if not ok:
        raise ValueError('%s must be a writable C-contiguous float64 array or tensor of %d values (shape %s)' % (name, size, (shape,)))
    return a


def _model_struct(arrs):
    """mpcqp_model with the fields of ``arrs`` (name -> prepared array or tensor); the others stay null = not given."""
    model = _lib.Model()
    for k, v in arrs.items():
        setattr(model, k, C.cast(_ptr(v), C.POINTER(C.c_double)))
    return model


def _prep(a, shape, name):
    """float64, C-contiguous, exact shape; returns an object that keeps the memory alive."""
    if a is None:
        raise ValueError('%s is required' % name)
    if hasattr(a, 'data_ptr'):
        import torch
        if a.numel() != int(np.prod(shape)):
            a = a.expand(shape)
        if a.dtype != torch.float64 or not a.is_contiguous() or tuple(a.shape) != tuple(shape):
            a = a.to(torch.float64).reshape(shape).contiguous()
        return a
    a = np.asarray(a, dtype=np.float64)
    if a.size == int(np.prod(shape)):
        return np.ascontiguousarray(a.reshape(shape))
    return np.ascontiguousarray(np.broadcast_to(a, shape))


BACKENDS = dict(auto=_lib.BACKEND_AUTO, sweeps=_lib.BACKEND_SWEEPS, dense=_lib.BACKEND_DENSE, bcr=_lib.BACKEND_BCR, bcr8=_lib.BACKEND_BCR8, bcrt=_lib.BACKEND_BCRT)
_forced = {}               # settings every handle made inside a ``forced_settings`` block gets (tests: one parity suite per KKT backend)


class forced_settings:
    """``with forced_settings(backend='bcr', tuning=TUNE_NO_BALANCE): ...`` -- every problem created inside the block gets these
    ``mpcqp_settings`` fields on top of what its caller asked for.  This is how the test-suite forces a KKT backend
    (``mpcqp_settings.backend``) through code that builds its own controllers; the library itself reads no environment variable."""

    def __init__(self, **kw):
        if isinstance(kw.get('backend'), str):
            kw['backend'] = BACKENDS[kw['backend']]
        self.kw = kw

    def __enter__(self):
        self.old = dict(_forced)
        _forced.update(self.kw)
        return self

    def __exit__(self, *exc):
        _forced.clear()
        _forced.update(self.old)
        return False


def _split_polish(kw):
    """(settings without the polish ones, the polish ones) of a settings dict."""
    kw = dict(kw)
    return kw, {k: kw.pop(k) for k in _POLISH_SETTINGS if k in kw}


def make_settings(**kw):
    L = _lib.load()
    s = _lib.Settings()
    L.mpcqp_default_settings(C.byref(s))
    kw = dict(kw, **_forced)
    if isinstance(kw.get('backend'), str):
        kw['backend'] = BACKENDS[kw['backend']]
    for k, v in kw.items():
        if k in _SETTING_NAMES:
            setattr(s, k, v)
        elif k in _IGNORED_SETTINGS:
            if k == 'scaled_termination' and v:
                raise NotImplementedError('scaled_termination=True is not implemented')
        else:
            raise TypeError('unknown solver setting %r' % k)
    return s


class Result:
    """Mimics osqp's results object as far as pyMPC reads it (mpc.py:301-327)."""

    class _Info:
        pass

    def __init__(self, x, y, info, status_str):
        self.x = x
        self.y = y
        self.info = Result._Info()
        self.info.status_val = int(info.status)
        self.info.status = status_str
        self.info.iter = int(info.iter)
        self.info.rho_updates = int(info.rho_updates)
        self.info.obj_val = float(info.obj_val)
        self.info.pri_res = float(info.pri_res)
        self.info.dua_res = float(info.dua_res)
        self.info.rho_estimate = float(info.rho)
        self.info.status_polish = 0               # osqp's name: 1 polished, -1 polishing rejected, 0 not performed (set by the caller)


class BatchProblem:
    """``batch`` independent MPC problems (nx, nu, Np, Nc) on GPU ``device``."""

    def __init__(self, batch, nx, nu, Np, Nc=None, device=0, stream=None, **settings):
        self._L = _lib.load()
        self._h = C.c_void_p()
        if self._L.mpcqp_device_count() <= 0:
            raise RuntimeError('pympc_amd needs an AMD GPU (no HIP device visible); there is no CPU fallback')
        self.batch, self.nx, self.nu, self.Np = int(batch), int(nx), int(nu), int(Np)
        self.Nc = int(Np if Nc is None else Nc)
        settings, polish = _split_polish(settings)
        self.settings = make_settings(**settings)
        rc = self._L.mpcqp_create(C.byref(self._h), int(device), self.batch, self.nx, self.nu, self.Np, self.Nc,
                                  C.byref(self.settings))
        if rc == -4:
            raise NotImplementedError(self._L.mpcqp_last_error().decode())
        _lib.check(rc, 'mpcqp_create')
        self._finish_init(stream)
        self._set_polish(**polish)

    @classmethod
    def from_matrices(cls, P, A, batch=1, device=0, stream=None, nx=None, nu=None, **settings):
        """The seam of mpc.py:266 with the matrices themselves (mpcqp_create_csc): the LIBRARY reads nx, nu, Np, Nc out of
        the sparsity patterns of P and A (scipy sparse, shared by the batch) and later, in ``setup_csc``, the controller
        data out of their values -- refusing anything that is not pyMPC's QP (``NotAnMPCQP``)."""
        import scipy.sparse as sp
        from .qp_recover import NotAnMPCQP
        self = cls.__new__(cls)
        self._L = _lib.load()
        self._h = C.c_void_p()
        self.batch = int(batch)
        settings, polish = _split_polish(settings)
        self.settings = make_settings(**settings)
        Pc, Ac = sp.csc_matrix(P), sp.csc_matrix(A)
        Pc.sort_indices(); Ac.sort_indices()
        self._csc = (Pc, Ac)
        pp, pi = np.ascontiguousarray(Pc.indptr, dtype=np.int64), np.ascontiguousarray(Pc.indices, dtype=np.int32)
        ap, ai = np.ascontiguousarray(Ac.indptr, dtype=np.int64), np.ascontiguousarray(Ac.indices, dtype=np.int32)
        rc = self._L.mpcqp_create_csc(C.byref(self._h), int(device), self.batch, int(Pc.shape[0]), int(Ac.shape[0]), _ptr(pp), _ptr(pi), _ptr(ap), _ptr(ai),
                                      int(nx or 0), int(nu or 0), C.byref(self.settings))
        if rc == -4:        # MPCQP_ERR_UNSUPPORTED: either not pyMPC's QP, or a valid one beyond what the device path implements
            msg = self._L.mpcqp_last_error().decode()
            if msg.startswith('mpcqp_create_csc: not an MPC QP'):
                raise NotAnMPCQP(msg)
            raise NotImplementedError(msg)
        if rc == -3:
            raise RuntimeError('pympc_amd needs an AMD GPU (no HIP device visible); there is no CPU fallback')
        _lib.check(rc, 'mpcqp_create_csc')
        d = [C.c_int() for _ in range(4)]
        _lib.check(self._L.mpcqp_get_shape(self._h, *[C.byref(v) for v in d]), 'mpcqp_get_shape')
        self.nx, self.nu, self.Np, self.Nc = (v.value for v in d)
        self._finish_init(stream)
        self._set_polish(**polish)
        return self

    def setup_csc(self, P_val, A_val, q, l, u):
        """Values of P [B, nnz(P)] and A [B, nnz(A)] in the index order given to ``from_matrices`` (sorted CSC), q [B, n], l, u [B, m]
        (host arrays): recovered, verified by a rebuild and set up by the library (mpcqp_setup_csc)."""
        from .qp_recover import NotAnMPCQP
        Pc, Ac = self._csc
        pv = _prep(P_val, (self.batch, Pc.nnz), 'P_val'); av = _prep(A_val, (self.batch, Ac.nnz), 'A_val')
        qa, la, ua = _prep(q, (self.batch, self.n), 'q'), _prep(l, (self.batch, self.m), 'l'), _prep(u, (self.batch, self.m), 'u')
        rc = self._L.mpcqp_setup_csc(self._h, _ptr(pv), _ptr(av), _ptr(qa), _ptr(la), _ptr(ua))
        if rc == -4:
            raise NotAnMPCQP(self._L.mpcqp_last_error().decode())
        _lib.check(rc, 'mpcqp_setup_csc')

    def _need(self, feature):
        """Raise NotImplementedError if the loaded library does not export ``feature`` (a key of _FEATURES); never a silent fallback."""
        has, what = _FEATURES[feature]
        if not has(self._L):
            raise NotImplementedError('this build of the solver library has ' + what)

    _hin = None                # (step_host of a single controller: input buffer, made on first use)
    _polish = None             # mpcqp_polish_settings of the handle (None: the library has no polishing, include/mpcqp_polish.h)

    def _set_polish(self, **kw):
        """Apply osqp's polish / delta / polish_refine_iter (mpcqp_set_polish).  Asking for polish=True of a library without
        include/mpcqp_polish.h raises NotImplementedError; it is never ignored."""
        if not _lib.has_polish(self._L):
            if kw.get('polish'):
                raise NotImplementedError('polish=True: this build of the solver library has no solution polishing (include/mpcqp_polish.h)')
            return
        if self._polish is None:
            self._polish = _lib.PolishSettings()
            self._L.mpcqp_polish_default_settings(C.byref(self._polish))
        if not kw:
            return
        for k, v in kw.items():
            setattr(self._polish, k, int(bool(v)) if k == 'polish' else v)
        _lib.check(self._L.mpcqp_set_polish(self._h, C.byref(self._polish)), 'mpcqp_set_polish')

    @property
    def polishing(self):
        """True if the solves of this problem are polished (polish=True)."""
        return self._polish is not None and bool(self._polish.polish)

    def polish(self):
        """Polish the last solve of every instance now (mpcqp_polish: stream-ordered), with this problem's delta / polish_refine_iter."""
        self._need('polish')
        _lib.check(self._L.mpcqp_polish(self._h), 'mpcqp_polish')

    def polish_status(self):
        """status_polish [batch] int32 of the last solve: 1 polished, -1 rejected, 0 not performed (mpcqp_get_polish_info; synchronises)."""
        out = np.zeros(self.batch, dtype=np.int32)
        if _lib.has_polish(self._L):
            _lib.check(self._L.mpcqp_get_polish_info(self._h, _ptr(out)), 'mpcqp_get_polish_info')
        return out

    # -- adjoint derivatives (include/mpcqp_adjoint.h) --------------------------------------------
    _adjoint = None            # mpcqp_adjoint_settings of the handle, once changed

    def set_adjoint(self, **kw):
        """The adjoint's own delta / refine_iter / extra_iter / weak_tol (mpcqp_set_adjoint); the polish settings are separate."""
        self._need('adjoint')
        if self._adjoint is None:
            self._adjoint = _lib.AdjointSettings()
            self._L.mpcqp_adjoint_default_settings(C.byref(self._adjoint))
        for k, v in kw.items():
            if k not in ('delta', 'refine_iter', 'weak_tol', 'extra_iter'):
                raise TypeError('unknown adjoint setting %r' % k)
            setattr(self._adjoint, k, v)
        _lib.check(self._L.mpcqp_set_adjoint(self._h, C.byref(self._adjoint)), 'mpcqp_set_adjoint')

    # rows of the last reference upload the library ACCEPTED (1 or Np+1): the shape d_xref / K_xref come back in.  It sizes the buffers the
    # library writes into, so it is only ever assigned after the uploading call has returned without an error.
    _xref_rows_last = 1

    def _out(self, like, shape):
        """An output array of the kind the inputs are: a torch tensor on ``like``'s device, else numpy."""
        if like is not None and hasattr(like, 'data_ptr'):
            import torch
            return torch.empty(shape, dtype=torch.float64, device=like.device)
        return np.empty(shape)

    def _model_grads(self, batch_sum):
        """(mpcqp_adjoint_model_io, its part of a gradient table): the model gradients per instance, or summed over the batch [1, ...]."""
        B, nx, nu = 1 if batch_sum else self.batch, self.nx, self.nu
        mo = _lib.AdjointModelIO()
        mo.struct_size, mo.batch_sum = C.sizeof(_lib.AdjointModelIO), int(bool(batch_sum))
        shapes = dict(Ad=(B, nx, nx), Bd=(B, nx, nu), Qx=(B, nx, nx), QxN=(B, nx, nx), Qu=(B, nu, nu), QDu=(B, nu, nu), eps_feas=(B,))
        return mo, {k: (mo, 'd_' + k, shape) for k, shape in shapes.items()}

    def _bound_grads(self, batch_sum):
        """(mpcqp_adjoint_bounds_io, its part of a gradient table): the bound gradients per instance, or summed over the batch [1, ...]."""
        B = 1 if batch_sum else self.batch
        bo = _lib.AdjointBoundsIO()
        bo.struct_size, bo.batch_sum = C.sizeof(_lib.AdjointBoundsIO), int(bool(batch_sum))
        return bo, {k: (bo, 'd_' + k, (B, self.nx if k in ('xmin', 'xmax') else self.nu)) for k in _lib.ADJOINT_BOUNDS_NAMES}

    def _grads_out(self, want, table, out, like):
        """The gradients named in ``want`` as a dict of arrays -- taken from ``out`` where it has them, else made like ``like`` -- each with its
        address put where ``table`` says: name -> (ctypes struct, field, shape)."""
        res = {}
        for k in want:
            if k not in table:
                raise TypeError('unknown gradient %r' % k)
            struct, field, shape = table[k]
            res[k] = _prep_out(out[k], shape, 'out[%r]' % k) if out is not None and k in out else self._out(like, shape)
            setattr(struct, field, _ptr(res[k]))
        return res

    def adjoint(self, g_w=None, g_u0=None, want=('x0', 'uminus1', 'xref', 'uref'), out=None, batch_sum=False):
        """Adjoint derivatives of the current solution (mpcqp_adjoint): for the seed ``g_w`` [B, n] = dL/dw and / or ``g_u0`` [B, nu] = dL/du_0
        returns a dict with the gradients named in ``want`` -- any of 'x0' [B, nx], 'uminus1' [B, nu], 'xref' [B, rows*nx] (shape of the
        last upload), 'uref' [B, nu], 'q' [B, n], 'l', 'u' [B, m], and of the model gradients 'Ad' [B, nx, nx], 'Bd' [B, nx, nu], 'Qx', 'QxN'
        [B, nx, nx], 'Qu', 'QDu' [B, nu, nu], 'eps_feas' [B] (mpcqp_adjoint_model, include/mpcqp_adjoint_model.h: the same call, the same
        single factorization; the weight gradients are those of a symmetric perturbation), and of the bound gradients 'xmin', 'xmax'
        [B, nx], 'umin', 'umax', 'Dumin', 'Dumax' [B, nu] (mpcqp_adjoint_bounds, include/mpcqp_adjoint_bounds.h: the multipliers of the active
        rows summed onto the bound each sits on).  ``batch_sum``: the model and bound gradients come summed
        over the batch, with a leading dimension of 1 -- one model shared by many states; the sum is formed on the device in a fixed order.
        'd' [B, rows*nx]: the gradient of the affine term in the shape it was set in (mpcqp_adjoint_affine, include_ext4/mpcqp_affine.h; beside a
        model or bound gradient it is a second call with the same seeds); without a term set it raises.
        Seeds may be numpy arrays or torch device tensors; the results are of the same kind (device tensors: stream-ordered, no wait), or
        are written into the arrays / tensors given in ``out`` (a dict by the same names).  The gradients are those of the active set the
        iterate implies; ``adjoint_info()`` reports weakly active rows."""
        if 'd' in want:
            self._need('affine')
        self._need('adjoint')
        if g_w is None and g_u0 is None:
            raise ValueError('adjoint: give g_w, g_u0 or both')
        B = self.batch
        like = g_w if g_w is not None else g_u0
        gw = _prep(g_w, (B, self.n), 'g_w') if g_w is not None else None
        gu = _prep(g_u0, (B, self.nu), 'g_u0') if g_u0 is not None else None
        io = _lib.AdjointIO()
        io.struct_size = C.sizeof(_lib.AdjointIO)
        io.g_w, io.g_u0 = _ptr(gw), _ptr(gu)
        shapes = dict(x0=(B, self.nx), uminus1=(B, self.nu), xref=(B, self._xref_rows_last * self.nx), uref=(B, self.nu),
                      q=(B, self.n), l=(B, self.m), u=(B, self.m))
        table = {k: (io, 'd_' + k, shape) for k, shape in shapes.items()}
        mo, mtable = self._model_grads(batch_sum)
        table.update(mtable)
        bo, btable = self._bound_grads(batch_sum)
        table.update(btable)
        want = list(want)
        want_d = 'd' in want
        if want_d:
            want.remove('d')
            drows = self.affine_rows()
            if not drows:
                raise RuntimeError("adjoint: want 'd' needs an affine term (set_affine)")
        if ('l' in want) != ('u' in want):
            want += ['l' if 'u' in want else 'u']
        model = any(k in mtable for k in want)
        bounds = any(k in btable for k in want)
        if model:
            self._need('adjoint_model')
        if bounds:
            self._need('adjoint_bounds')
        res = self._grads_out(want, table, out, like)
        self._keep = [gw, gu, res]
        if want_d:
            shape = (B, drows * self.nx)
            res['d'] = _prep_out(out['d'], shape, "out['d']") if out is not None and 'd' in out else self._out(like, shape)
            seeds = io
            if model or bounds:                   # (mpcqp_adjoint_affine takes mpcqp_adjoint's outputs only: the seeds again, for the term alone)
                seeds = _lib.AdjointIO()
                seeds.struct_size, seeds.g_w, seeds.g_u0 = C.sizeof(_lib.AdjointIO), _ptr(gw), _ptr(gu)
            _lib.check(self._L.mpcqp_adjoint_affine(self._h, C.byref(seeds), _ptr(res['d'])), 'mpcqp_adjoint_affine')
            if not (model or bounds):
                return res
        if bounds:
            _lib.check(self._L.mpcqp_adjoint_bounds(self._h, C.byref(io), C.byref(mo) if model else None, C.byref(bo)), 'mpcqp_adjoint_bounds')
        elif model:
            _lib.check(self._L.mpcqp_adjoint_model(self._h, C.byref(io), C.byref(mo)), 'mpcqp_adjoint_model')
        else:                                     # (without a model gradient: the call as it always was)
            _lib.check(self._L.mpcqp_adjoint(self._h, C.byref(io)), 'mpcqp_adjoint')
        return res

    def gains(self, want=('x0', 'uminus1', 'xref', 'uref'), like=None):
        """Jacobians of the first input u_0 of the current solution (mpcqp_gains: one factorization, nu seeds): dict with 'x0' [B, nu, nx],
        'uminus1' [B, nu, nu], 'xref' [B, nu, rows*nx], 'uref' [B, nu, nu] as named in ``want``; numpy, or torch tensors on the device
        of ``like``.  On a problem that has an affine term (``set_affine``), where the library has the call (mpcqp_gains_affine,
        include_ext5/mpcqp_rollout_affine.h: the same factorization and seeds), also 'd' [B, nu, rows*nx] = d u_0 / d d; without a term the dict is
        as it always was."""
        self._need('adjoint')
        B, nu = self.batch, self.nu
        shapes = dict(x0=(B, nu, self.nx), uminus1=(B, nu, nu), xref=(B, nu, self._xref_rows_last * self.nx), uref=(B, nu, nu))
        res = {k: self._out(like, shapes[k]) for k in want}
        self._keep = [res]
        drows = self.affine_rows() if _lib.has_rollout_affine(self._L) and _lib.has_affine(self._L) else 0
        if drows:
            res['d'] = self._out(like, (B, nu, drows * self.nx))
            _lib.check(self._L.mpcqp_gains_affine(self._h, *[_ptr(res.get(k)) for k in ('x0', 'uminus1', 'xref', 'uref', 'd')]), 'mpcqp_gains_affine')
            return res
        _lib.check(self._L.mpcqp_gains(self._h, *[_ptr(res.get(k)) for k in ('x0', 'uminus1', 'xref', 'uref')]), 'mpcqp_gains')
        return res

    def adjoint_info(self):
        """(n_active, n_weak, status) [batch] int32 of the last adjoint() / gains() (mpcqp_get_adjoint_info; synchronises): status 1 computed,
        0 the instance's solve did not end 'solved', -1 the factorization broke (outputs zero in both cases); n_weak > 0: rows on a bound
        with a zero multiplier -- the control law has a kink there and the result is a one-sided derivative."""
        self._need('adjoint')
        out = [np.zeros(self.batch, dtype=np.int32) for _ in range(3)]
        _lib.check(self._L.mpcqp_get_adjoint_info(self._h, *[_ptr(o) for o in out]), 'mpcqp_get_adjoint_info')
        return tuple(out)

    # -- a rollout with a tape and its reverse sweep (include/mpcqp_rollout.h) ---------------------
    _tape = None               # the _Tape the handle holds (None: none)
    rollout_count = 0          # rollouts made so far (pympc_amd.torch_layer: is the tape still the one of a forward?)

    def _taped_loop(self, nsteps, w, Ap, Bp, out, xref_traj, model_traj=None, estimator=None, L_traj=None, affine=None):
        """The taped loop of every form: ``_loop`` through mpcqp_rollout, _est, _tv or _tv_est as the options say -- or, with ``affine = (d_traj or
        None, d_hold)``, mpcqp_rollout_affine -- then the record of the tape."""
        entry = 'mpcqp_rollout' + ('_tv' if model_traj is not None else '') + ('_est' if estimator is not None else '')
        aff = None
        if affine is not None:
            entry, (d_traj, d_hold) = 'mpcqp_rollout_affine', affine
            rows = self.affine_rows()                 # (of the handle's own term: the tape's where there is no schedule)
            if d_traj is None and not rows:
                raise RuntimeError('rollout_affine: no d_traj given and no affine term set (set_affine); rollout is the taped loop without one')
            res = self._loop(entry, nsteps, w=w, Ap=Ap, Bp=Bp, out=out, xref_traj=xref_traj, model_traj=model_traj, d_traj=d_traj, d_hold=d_hold)
            if d_traj is not None:
                rows, hold = int(np.prod(tuple(d_traj.shape)[2:])) // self.nx, int(d_hold)
                aff = (rows, hold, (int(nsteps) + hold - 1) // hold + 1)
            else:
                aff = (rows, 0, 1)
        else:
            res = self._loop(entry, nsteps, w=w, Ap=Ap, Bp=Bp, out=out, xref_traj=xref_traj, estimator=estimator, model_traj=model_traj, L_traj=L_traj)
        sched = None
        if model_traj is not None:
            hold = int(model_traj[2])
            sched = (hold, (int(nsteps) + hold - 1) // hold, model_traj[0] is not None, model_traj[1] is not None)
        self._tape = _Tape(int(nsteps), self._xref_rows_last, int(tuple(estimator['C'].shape)[-2]) if estimator is not None else 0, sched, aff)
        self.rollout_count += 1
        return res

    def rollout(self, nsteps, w=None, Ap=None, Bp=None, out=None, xref_traj=None):
        """``mpc_run`` that keeps a tape (mpcqp_rollout): the same arguments and results, one closed-loop launch per step, and afterwards
        ``rollout_adjoint`` can push a loss on the trajectory back through the loop.  No estimator, no model schedule."""
        self._need('rollout')
        return self._taped_loop(nsteps, w, Ap, Bp, out, xref_traj)

    def rollout_est(self, nsteps, estimator, w=None, Ap=None, Bp=None, xref_traj=None, out=None):
        """``mpc_run(estimator=dict(C=, L=, x_true=, v=))`` that keeps a tape (mpcqp_rollout_est): the same arguments and results
        (``x, u, status, iter, xhat, y``), and afterwards ``rollout_adjoint`` -- with ``g_xhat``, ``g_y`` and the gradients 'eta', 'C', 'L', 'v',
        'Ae', 'Be' on top -- pushes a loss on the trajectory back through controller, plant and estimator."""
        self._need('rollout_est')
        if estimator is None:
            raise ValueError('rollout_est: an estimator dict(C=, L=, x_true=, v=) is needed (rollout is the taped loop without one)')
        return self._taped_loop(nsteps, w, Ap, Bp, out, xref_traj, estimator=estimator)

    def rollout_tv(self, nsteps, model_traj, w=None, Ap=None, Bp=None, out=None, xref_traj=None):
        """``mpc_run(model_traj=)`` that keeps a tape (mpcqp_rollout_tv, include_ext/mpcqp_rollout_tv.h): the same arguments and results, one
        closed-loop launch per step, and a tape that remembers every model it was made under -- slot 0: the model the call began with, slot
        e + 1: schedule entry e.  Afterwards ``rollout_adjoint`` differentiates the loop with respect to every one of them."""
        self._need('rollout_tv')
        if model_traj is None:
            raise ValueError('rollout_tv: a model_traj = (Ad, Bd, hold) is needed (rollout is the taped loop on one model)')
        return self._taped_loop(nsteps, w, Ap, Bp, out, xref_traj, model_traj=model_traj)

    def mpc_run_tv_est(self, nsteps, model_traj, estimator, L_traj=None, w=None, Ap=None, Bp=None, out=None, xref_traj=None):
        """``mpc_run`` with an estimator AND a model schedule (mpcqp_mpc_loop_tv_est, include_ext2/mpcqp_rollout_tv_est.h): the output-feedback
        loop in which entry ``k // hold`` of ``model_traj`` replaces Ad / Bd at the start of step k -- for the controller, the estimator and,
        without ``Ap``/``Bp``, the plant -- and, with ``L_traj`` [nentries, B, nx, ny], entry ``k // hold`` of it is the observer gain of step k
        (``estimator['L']`` may then be None).  Results as ``mpc_run`` with an estimator."""
        self._need('rollout_tv_est')
        if model_traj is None or estimator is None:
            raise ValueError('mpc_run_tv_est: a model_traj = (Ad, Bd, hold) and an estimator dict(C=, L=, x_true=, v=) are both needed')
        return self._loop('mpcqp_mpc_loop_tv_est', nsteps, w=w, Ap=Ap, Bp=Bp, out=out, xref_traj=xref_traj, estimator=estimator, model_traj=model_traj, L_traj=L_traj)

    def rollout_tv_est(self, nsteps, model_traj, estimator, L_traj=None, w=None, Ap=None, Bp=None, out=None, xref_traj=None):
        """``mpc_run_tv_est`` that keeps a tape (mpcqp_rollout_tv_est): the same arguments and results, one closed-loop launch per step, and a
        tape with the model slots of ``rollout_tv``, the plant states and measurements of ``rollout_est`` and the gain of every entry.
        Afterwards ``rollout_adjoint`` differentiates the loop through controller, plant and estimator, entry by entry."""
        self._need('rollout_tv_est')
        if model_traj is None or estimator is None:
            raise ValueError('rollout_tv_est: a model_traj = (Ad, Bd, hold) and an estimator dict(C=, L=, x_true=, v=) are both needed')
        return self._taped_loop(nsteps, w, Ap, Bp, out, xref_traj, model_traj=model_traj, estimator=estimator, L_traj=L_traj)

    def rollout_affine(self, nsteps, d_traj=None, d_hold=1, model_traj=None, w=None, Ap=None, Bp=None, out=None, xref_traj=None):
        """``mpc_run(d_traj=, d_hold=, model_traj=)`` that keeps a tape (mpcqp_rollout_affine, include_ext5/mpcqp_rollout_affine.h): the same arguments
        and results, one closed-loop launch per step, and a tape that remembers the affine term of every solve as slots -- slot 0: the term the
        problem held when the call began (zeros if none), slot e + 1: entry e of ``d_traj``; tape entry k was solved under slot 0 for k = 0 and
        ``1 + (k - 1) // d_hold`` beyond.  ``d_traj=None``: the problem's own term (``set_affine``) throughout, one slot.  Afterwards
        ``rollout_adjoint`` differentiates the loop with respect to the terms too ('d0', 'd_traj').  No estimator."""
        self._need('rollout_affine')
        return self._taped_loop(nsteps, w, Ap, Bp, out, xref_traj, model_traj=model_traj, affine=(d_traj, d_hold))

    def rollout_affine_tape_bytes(self, nsteps, rows, d_hold=0, model_hold=0):
        """Device memory the tape of ``rollout_affine`` takes (mpcqp_rollout_affine_tape_bytes; ``d_hold`` 0: no ``d_traj``, ``model_hold`` 0: no
        ``model_traj``)."""
        self._need('rollout_affine')
        return self._tape_bytes('mpcqp_rollout_affine_tape_bytes', nsteps, model_hold, d_hold, rows)

    def rollout_affine_slot(self, s):
        """The affine term of slot s on the tape of a ``rollout_affine`` [B, rows, nx] (mpcqp_rollout_affine_get_slot; verification)."""
        self._need('rollout_affine')
        if self._tape is None or self._tape.aff is None:
            raise RuntimeError('rollout_affine_slot: the last rollout was not a rollout_affine')
        d = np.empty((self.batch, self._tape.aff[0], self.nx))
        _lib.check(self._L.mpcqp_rollout_affine_get_slot(self._h, int(s), _ptr(d)), 'mpcqp_rollout_affine_get_slot')
        return d

    def _tape_bytes(self, fn, *sizes):
        """What the library's ``fn`` says a tape of these sizes takes."""
        v = C.c_int64()
        _lib.check(getattr(self._L, fn)(self._h, *[int(s) for s in sizes], C.byref(v)), fn)
        return v.value

    def rollout_tv_est_tape_bytes(self, nsteps, hold, ny):
        """Device memory the tape of ``rollout_tv_est`` takes (mpcqp_rollout_tv_est_tape_bytes)."""
        self._need('rollout_tv_est')
        return self._tape_bytes('mpcqp_rollout_tv_est_tape_bytes', nsteps, hold, ny)

    def rollout_tv_est_gain(self, e):
        """The observer gain of schedule entry e on the tape of a ``rollout_tv_est`` as the sweep reads it [B, nx, ny]
        (mpcqp_rollout_tv_est_get_gain; verification)."""
        self._need('rollout_tv_est')
        Lg = np.empty((self.batch, self.nx, max(self._tape.ny if self._tape else 0, 1)))
        _lib.check(self._L.mpcqp_rollout_tv_est_get_gain(self._h, int(e), _ptr(Lg)), 'mpcqp_rollout_tv_est_get_gain')
        return Lg

    def rollout_tv_tape_bytes(self, nsteps, hold):
        """Device memory the tape of ``nsteps`` steps under a schedule with this ``hold`` takes (mpcqp_rollout_tv_tape_bytes)."""
        self._need('rollout_tv')
        return self._tape_bytes('mpcqp_rollout_tv_tape_bytes', nsteps, hold)

    def rollout_tv_slot(self, s):
        """Model slot s of a scheduled tape as the sweep reads it (mpcqp_rollout_tv_get_slot; verification): dict(model [B, model doubles] the
        blob (Ad | Bd | xmin | xmax | umin | umax | Dumin | Dumax | uref | eps_feas | Qx | QxN | Qu | QDu), D [B, n], E [B, m], c [B])."""
        self._need('rollout_tv')
        B, nx, nu = self.batch, self.nx, self.nu
        r = dict(model=np.empty((B, 3 * nx * nx + nx * nu + 2 * nu * nu + 2 * nx + 5 * nu + 1)), D=np.empty((B, self.n)), E=np.empty((B, self.m)), c=np.empty(B))
        _lib.check(self._L.mpcqp_rollout_tv_get_slot(self._h, int(s), *[_ptr(r[n]) for n in ('model', 'D', 'E', 'c')]), 'mpcqp_rollout_tv_get_slot')
        return r

    def rollout_tape_bytes(self, nsteps, ny=0):
        """Device memory a tape of ``nsteps`` steps takes (mpcqp_rollout_tape_bytes; with ``ny`` outputs: mpcqp_rollout_est_tape_bytes)."""
        self._need('rollout')
        if ny:
            self._need('rollout_est')
            return self._tape_bytes('mpcqp_rollout_est_tape_bytes', nsteps, ny)
        return self._tape_bytes('mpcqp_rollout_tape_bytes', nsteps)

    def rollout_release(self):
        """Free the tape (mpcqp_rollout_release)."""
        self._need('rollout')
        _lib.check(self._L.mpcqp_rollout_release(self._h), 'mpcqp_rollout_release')
        self._tape = None

    def rollout_adjoint(self, g_x=None, g_u=None, want=('lam', 'uminus1', 'uref', 'xref'), out=None, batch_sum=False, no_reuse=False, g_xhat=None, g_y=None):
        """The reverse sweep over the tape of the last ``rollout`` (mpcqp_rollout_adjoint): for ``g_x`` [K+1, B, nx] = dL/dx_k and / or
        ``g_u`` [K, B, nu] = dL/du_k returns a dict with the gradients named in ``want`` -- 'lam' [K+1, B, nx] (lam[0] = dL/dx0,
        lam[k+1] = dL/dw[k]), 'uminus1' [B, nu], 'uref' [B, nu], 'xref' [K, B, rows*nx] (entry k: the reference step k was solved with),
        'Ap' [B, nx, nx], 'Bp' [B, nx, nu] (the plant path alone) and the model gradients of ``adjoint`` ('Ad', 'Bd', 'Qx', 'QxN', 'Qu', 'QDu',
        'eps_feas'; ``batch_sum`` as there) and bound gradients ('xmin', 'xmax', 'umin', 'umax', 'Dumin', 'Dumax': mpcqp_rollout_adjoint_bounds),
        summed over the steps.  ``no_reuse``: factor at every step (the same bits, for measurements).
        numpy in, numpy out; torch device tensors in, device tensors out (stream-ordered, no wait).
        On the tape of a ``rollout_est`` (mpcqp_rollout_adjoint_est): ``g_xhat`` [K+1, B, nx] = dL/dxhat_k and ``g_y`` [K, B, ny] = dL/dy_k are
        seeds too (any one of the four is enough), and ``want`` may name 'eta' [K+1, B, nx] (eta[0] = dL/dxhat_0), 'C' [B, ny, nx],
        'L' [B, nx, ny], 'v' [K, B, ny], 'Ae' [B, nx, nx], 'Be' [B, nx, nu] (the estimator path alone); on a state-feedback tape they raise.
        On the tape of a ``rollout_tv`` (mpcqp_rollout_adjoint_tv): ``want`` may name 'Ad_traj' [nseg, B, nx, nx], 'Bd_traj' [nseg, B, nx, nu] --
        entry e: the solve path of the solves made under schedule entry e -- and 'Ap_traj', 'Bp_traj' of the same shapes: the plant path of
        the steps entry e was in force.  'Ad', 'Bd' are then the solve path of the model the call began with, plus that of all entries for a
        matrix the schedule did not give (it never changed); 'Ap', 'Bp' the sum over the entries.  ``batch_sum`` sums these over the
        instances too ([nseg, 1, ..] and [1, ..]).  On any other tape the four ``_traj`` names raise.
        On the tape of a ``rollout_tv_est`` (mpcqp_rollout_adjoint_tv_est): everything the scheduled sweep and the estimator sweep take, and
        'Ae_traj' [nseg, B, nx, nx], 'Be_traj' [nseg, B, nx, nu], 'L_traj' [nseg, B, nx, ny] -- the estimator path of the steps entry e was in
        force; 'Ae', 'Be', 'L' are their sums over the entries."""
        aff_names = ('d0', 'd_traj')
        if any(k in aff_names for k in want):
            self._need('rollout_affine')
        self._need('rollout')
        tape = self._tape
        ny, sched = (tape.ny, tape.sched) if tape is not None else (0, None)
        aff = tape.aff if tape is not None else None
        est_seeds = g_xhat is not None or g_y is not None
        tv_est_names, tv_names, est_names = ('Ae_traj', 'Be_traj', 'L_traj'), ('Ad_traj', 'Bd_traj', 'Ap_traj', 'Bp_traj'), ('eta', 'C', 'L', 'v', 'Ae', 'Be')
        named = lambda names: any(k in names for k in want)
        # (what was asked for, what the tape must have for it, what is said where it has not); on a scheduled tape without an estimator the
        # estimator's gradients are unknown names like any other
        refusals = ((named(aff_names), aff is not None, 'the gradients %s need the tape of a rollout_affine' % ', '.join(aff_names)),
                    ('d_traj' in want, aff is not None and aff[1] > 0, "the gradient d_traj needs a rollout_affine that was given a d_traj (this one ran under the problem's own term: 'd0')"),
                    (named(tv_est_names), sched is not None and ny, 'the gradients %s need the tape of a rollout_tv_est' % ', '.join(tv_est_names)),
                    (named(tv_names), sched is not None, 'the gradients %s need the tape of a rollout_tv (this one was made on one model)' % ', '.join(tv_names)),
                    (est_seeds and sched is not None, ny, 'g_xhat, g_y need the tape of a rollout_est (this one has no estimator)'),
                    ((est_seeds or named(est_names)) and sched is None, ny,
                     'g_xhat, g_y and the gradients %s need the tape of a rollout_est (this one has no estimator)' % ', '.join(est_names)))
        for asked, has, msg in refusals:
            if tape is not None and asked and not has:
                raise RuntimeError('rollout_adjoint: ' + msg)
        if g_x is None and g_u is None and not est_seeds:
            raise ValueError('rollout_adjoint: give g_x, g_u or both' + (', or g_xhat, g_y' if ny else ''))
        if tape is None:
            raise RuntimeError('rollout_adjoint: no rollout has been made (mpcqp_rollout)')
        self._need('rollout_affine' if aff is not None else 'rollout' + ('_tv' if sched is not None else '') + ('_est' if ny else ''))
        K, rows = tape.K, tape.rows
        B, nx, nu = self.batch, self.nx, self.nu
        like = next(g for g in (g_x, g_u, g_xhat, g_y) if g is not None)
        gx = _prep(g_x, (K + 1, B, nx), 'g_x') if g_x is not None else None
        gu = _prep(g_u, (K, B, nu), 'g_u') if g_u is not None else None
        gxh = _prep(g_xhat, (K + 1, B, nx), 'g_xhat') if g_xhat is not None else None
        gy = _prep(g_y, (K, B, ny), 'g_y') if g_y is not None else None
        io = _lib.RolloutAdjointIO()
        io.struct_size, io.no_reuse = C.sizeof(_lib.RolloutAdjointIO), int(bool(no_reuse))
        io.G_x, io.G_u = _ptr(gx), _ptr(gu)
        eo = _lib.RolloutEstIO()
        eo.struct_size = C.sizeof(_lib.RolloutEstIO)
        eo.G_xhat, eo.G_y = _ptr(gxh), _ptr(gy)
        table = dict(lam=(io, 'lam', (K + 1, B, nx)), uminus1=(io, 'd_uminus1', (B, nu)), uref=(io, 'd_uref', (B, nu)),
                     xref=(io, 'd_xref', (K, B, rows * nx)), Ap=(io, 'd_Ap', (B, nx, nx)), Bp=(io, 'd_Bp', (B, nx, nu)))
        if ny:
            table.update(eta=(eo, 'eta', (K + 1, B, nx)), C=(eo, 'd_C', (B, ny, nx)), L=(eo, 'd_L', (B, nx, ny)), v=(eo, 'd_v', (K, B, ny)),
                         Ae=(eo, 'd_Ae', (B, nx, nx)), Be=(eo, 'd_Be', (B, nx, nu)))
        mo, mtable = self._model_grads(batch_sum)
        table.update(mtable)
        bo, btable = self._bound_grads(batch_sum)
        table.update(btable)
        bounds = any(k in btable for k in want)
        if bounds:
            self._need('adjoint_bounds')
        # what a schedule splits: name -> (field of mpcqp_rollout_tv_io / _tv_est_io, its leading dimension, its columns, how the answer is read
        # from it).  These names are views and sums of the call's own per-slot / per-entry buffers: ``out`` serves the other names only
        split, to, xo = {}, _lib.RolloutTVIO(), _lib.RolloutTVEstIO()
        to.struct_size, xo.struct_size = C.sizeof(_lib.RolloutTVIO), C.sizeof(_lib.RolloutTVEstIO)
        if sched is not None:
            _, nseg, gave_Ad, gave_Bd = sched
            entries, total = (lambda a: a), (lambda a: a.sum(0))
            whole = lambda gave: (lambda a: a[0] if gave else a.sum(0))      # (slot 0: the model the call began with; a matrix the schedule left alone never changed)
            split = dict(Ad_traj=('d_Ad_slots', nseg + 1, nx, lambda a: a[1:]), Bd_traj=('d_Bd_slots', nseg + 1, nu, lambda a: a[1:]),
                         Ad=('d_Ad_slots', nseg + 1, nx, whole(gave_Ad)), Bd=('d_Bd_slots', nseg + 1, nu, whole(gave_Bd)))
            for k, cols in (('Ap', nx), ('Bp', nu)) + ((('Ae', nx), ('Be', nu), ('L', ny)) if ny else ()):      # (per entry; the unsuffixed name: the sum over the entries)
                split[k + '_traj'], split[k] = ('d_%s_entries' % k, nseg, cols, entries), ('d_%s_entries' % k, nseg, cols, total)
        ao = _lib.RolloutAffineIO()
        ao.struct_size = C.sizeof(_lib.RolloutAffineIO)
        if aff is not None:                       # (the terms' gradients per slot [nslots, B, rows*nx]: slot 0 is 'd0', the slots behind it 'd_traj')
            split.update(d0=('d_d_slots', aff[2], None, lambda a: a[0]), d_traj=('d_d_slots', aff[2], None, lambda a: a[1:]))
        bufs = {}
        for k in want:
            if k in split and split[k][0] not in bufs:
                field, lead, cols, _ = split[k]
                bufs[field] = self._out(like, (lead, B, aff[0] * nx) if cols is None else (lead, B, nx, cols))
                setattr(ao if hasattr(ao, field) else xo if hasattr(xo, field) else to, field, _ptr(bufs[field]))
        res = self._grads_out([k for k in want if k not in split], table, out, like)
        self._keep = [gx, gu, gxh, gy, res, bufs]
        # which C function, with which structs (None: not passed)
        if aff is not None:
            fn, structs = 'mpcqp_rollout_adjoint_affine', (io, mo, bo if bounds else None, to if sched is not None else None, ao)
        elif sched is not None:
            fn, structs = ('mpcqp_rollout_adjoint_tv_est', (io, eo, mo, bo, to, xo)) if ny else ('mpcqp_rollout_adjoint_tv', (io, mo, bo, to))
        elif bounds:
            fn, structs = 'mpcqp_rollout_adjoint_bounds', (io, eo if ny else None, mo, bo)
        else:
            fn, structs = ('mpcqp_rollout_adjoint_est', (io, eo, mo)) if ny else ('mpcqp_rollout_adjoint', (io, mo))
        _lib.check(getattr(self._L, fn)(self._h, *[None if s is None else C.byref(s) for s in structs]), fn)
        for k in want:
            if k in split:
                a = bufs[split[k][0]]
                res[k] = split[k][3](a.sum(1)[:, None] if batch_sum else a)      # ('d0': [B, ..] or [1, ..])
        return res

    def rollout_info(self):
        """(n_active [K, B], n_weak [K, B], status [K, B], n_factor [B]) int32 of the last ``rollout_adjoint`` (mpcqp_get_rollout_info;
        synchronises): per tape entry as ``adjoint_info``; n_factor: the factorizations the sweep made."""
        self._need('rollout')
        if self._tape is None:
            raise RuntimeError('rollout_info: no rollout has been made (mpcqp_rollout)')
        K = self._tape.K
        out = [np.zeros((K, self.batch), dtype=np.int32) for _ in range(3)] + [np.zeros(self.batch, dtype=np.int32)]
        _lib.check(self._L.mpcqp_get_rollout_info(self._h, *[_ptr(o) for o in out]), 'mpcqp_get_rollout_info')
        return tuple(out)

    def rollout_tape(self, k):
        """Tape entry k (mpcqp_rollout_get_tape; verification): dict(x [B, n], z, y [B, m], step [B, nx + nu + rows*nx] = (x_k | the u_{-1}
        the solve was made with | xref), status [B])."""
        self._need('rollout')
        if self._tape is None:
            raise RuntimeError('rollout_tape: no rollout has been made (mpcqp_rollout)')
        B, rows, ny = self.batch, self._tape.rows, self._tape.ny
        r = dict(x=np.empty((B, self.n)), z=np.empty((B, self.m)), y=np.empty((B, self.m)),
                 step=np.empty((B, self.nx + self.nu + rows * self.nx)), status=np.zeros(B, dtype=np.int32))
        _lib.check(self._L.mpcqp_rollout_get_tape(self._h, int(k), *[_ptr(r[n]) for n in ('x', 'z', 'y', 'step', 'status')]), 'mpcqp_rollout_get_tape')
        if ny:                                    # (a rollout_est: the step data begin with the estimate, the plant state and the measurement are beside it)
            r.update(x_plant=np.empty((B, self.nx)), y_meas=np.empty((B, ny)))
            _lib.check(self._L.mpcqp_rollout_get_tape_est(self._h, int(k), _ptr(r['x_plant']), _ptr(r['y_meas'])), 'mpcqp_rollout_get_tape_est')
        if self._tape.aff is not None:            # (a rollout_affine: the term the entry was solved with lies behind the rest of its step data)
            r['d'] = np.empty((B, self._tape.aff[0], self.nx))
            _lib.check(self._L.mpcqp_rollout_affine_get_tape(self._h, int(k), _ptr(r['d'])), 'mpcqp_rollout_affine_get_tape')
        return r

    def _finish_init(self, stream):
        n, m, fd, nnzL = C.c_int(), C.c_int(), C.c_int64(), C.c_int64()
        _lib.check(self._L.mpcqp_get_dims(self._h, C.byref(n), C.byref(m), C.byref(fd), C.byref(nnzL)), 'mpcqp_get_dims')
        self.n, self.m, self.factor_doubles, self.nnzL = n.value, m.value, fd.value, nnzL.value
        if stream is not None:
            _lib.check(self._L.mpcqp_set_stream(self._h, C.c_void_p(int(stream))), 'mpcqp_set_stream')
        self._keep = []

    def close(self):
        if getattr(self, '_h', None) and self._h.value:
            self._L.mpcqp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- reference-shaped calls ---------------------------------------------------------------
    def setup(self, Ad, Bd, Qx, QxN, Qu, QDu, xmin, xmax, umin, umax, Dumin, Dumax, uref, eps_feas,
              x0, uminus1, xref):
        B, nx, nu = self.batch, self.nx, self.nu
        xref_rows = self._xref_rows(xref)
        given = dict(Ad=Ad, Bd=Bd, Qx=Qx, QxN=QxN, Qu=Qu, QDu=QDu, xmin=xmin, xmax=xmax, umin=umin, umax=umax, Dumin=Dumin, Dumax=Dumax,
                     uref=uref, eps_feas=eps_feas)
        arrs = {k: _prep(given[k], shape, k) for k, shape in self._model_shapes().items()}
        model = _model_struct(arrs)
        x0a = _prep(x0, (B, nx), 'x0')
        uma = _prep(uminus1, (B, nu), 'uminus1')
        xra = _prep(xref, (B, xref_rows * nx), 'xref')
        self._keep = [arrs, x0a, uma, xra]
        _lib.check(self._L.mpcqp_setup(self._h, C.byref(model), _ptr(x0a), _ptr(uma), _ptr(xra), xref_rows), 'mpcqp_setup')
        self._xref_rows_last = xref_rows
        _lib.check(self._L.mpcqp_synchronize(self._h), 'mpcqp_synchronize')
        self._keep = []

    def setup_qp(self, Ad, Bd, Qx, QxN, Qu, QDu, eps_feas, q, l, u, uref=None):
        """The solver seam of mpc.py:266 with caller-built vectors (mpcqp_setup_qp): the matrices enter through the
        blocks they are made of (pympc_amd.qp_recover reads them out of a reference-layout P, A), q [B,n], l, u [B,m]
        verbatim."""
        shapes = self._model_shapes()
        given = dict(Ad=Ad, Bd=Bd, Qx=Qx, QxN=QxN, Qu=Qu, QDu=QDu, eps_feas=eps_feas)
        if uref is not None:
            given['uref'] = uref
        arrs = {k: _prep(v, shapes[k], k) for k, v in given.items()}
        model = _model_struct(arrs)
        qa, la, ua = _prep(q, (self.batch, self.n), 'q'), self._bound(l, 'l'), self._bound(u, 'u')
        _lib.check(self._L.mpcqp_setup_qp(self._h, C.byref(model), _ptr(qa), _ptr(la), _ptr(ua)), 'mpcqp_setup_qp')
        _lib.check(self._L.mpcqp_synchronize(self._h), 'mpcqp_synchronize')

    def _bound(self, v, name):
        return None if v is None else _prep(v, (self.batch, self.m), name)

    def _model_shapes(self):
        B, nx, nu = self.batch, self.nx, self.nu
        return dict(Ad=(B, nx, nx), Bd=(B, nx, nu), Qx=(B, nx, nx), QxN=(B, nx, nx), Qu=(B, nu, nu), QDu=(B, nu, nu),
                    xmin=(B, nx), xmax=(B, nx), umin=(B, nu), umax=(B, nu), Dumin=(B, nu), Dumax=(B, nu), uref=(B, nu), eps_feas=(B, 1))

    def update_model(self, **fields):
        """A new model under a problem that is in use (mpcqp_update_model, include/mpcqp_model.h): the given fields -- names and shapes as in
        ``setup``, numpy arrays or torch device tensors, None = unchanged -- replace the problem's, the device re-equilibrates, rebuilds the rho
        vector, refactors and keeps the iterate: the next solve warm-starts from it exactly as setup + warm_start(x, y) would.  Stream-ordered
        (no wait) when every field is device memory."""
        self._need('model_update')
        shapes = self._model_shapes()
        for k in fields:
            if k not in shapes:
                raise TypeError('unknown model field %r' % k)
        arrs = {k: _prep(v, shapes[k], k) for k, v in fields.items() if v is not None}
        if not arrs:
            raise ValueError('update_model: give at least one model field')
        model = _model_struct(arrs)
        self._keep = [arrs]                    # (device tensors: alive until the stream has read them -- at least until the next call)
        _lib.check(self._L.mpcqp_update_model(self._h, C.byref(model)), 'mpcqp_update_model')

    def update_vectors(self, q=None, l=None, u=None):
        """osqp's update(q=, l=, u=) (mpc.py:454) with caller-built vectors.  q may be None (unchanged); l and u go together --
        both or neither: the equality rows l[:nx] == u[:nx] carry x0 (the library refuses one without the other)."""
        if (l is None) != (u is None):
            raise ValueError('update_vectors: give l and u together (the equality rows l[:nx] == u[:nx] carry x0)')
        qa = None if q is None else _prep(q, (self.batch, self.n), 'q')
        la, ua = self._bound(l, 'l'), self._bound(u, 'u')
        _lib.check(self._L.mpcqp_update_vectors(self._h, _ptr(qa), _ptr(la), _ptr(ua)), 'mpcqp_update_vectors')

    def _xref_rows(self, xref):
        shape = tuple(xref.shape)
        per = math.prod(shape[1:]) if len(shape) > 1 and shape[0] == self.batch else math.prod(shape)
        if per == self.nx:
            return 1
        if per == (self.Np + 1) * self.nx:
            return self.Np + 1
        raise ValueError('xref must hold nx or (Np+1)*nx values per instance')

    def update(self, x0=None, uminus1=None, xref=None):
        B, nx, nu = self.batch, self.nx, self.nu
        rows = 1
        a = _prep(x0, (B, nx), 'x0') if x0 is not None else None
        b = _prep(uminus1, (B, nu), 'uminus1') if uminus1 is not None else None
        c = None
        if xref is not None:
            rows = self._xref_rows(xref)
            c = _prep(xref, (B, rows * nx), 'xref')
        self._keep = [a, b, c]
        _lib.check(self._L.mpcqp_update(self._h, _ptr(a), _ptr(b), _ptr(c), rows), 'mpcqp_update')
        if xref is not None:
            self._xref_rows_last = rows

    # -- the affine term of the prediction model (include_ext4/mpcqp_affine.h) --------------------
    def set_affine(self, d):
        """The affine term of the prediction model x+ = Ad x + Bd u + d_k (mpcqp_set_affine): ``d`` [B, nx] -- one offset for every stage -- or
        [B, Np, nx] (row k: the step k -> k+1), numpy or a torch device tensor (stream-ordered); ``None`` clears it.  Step data like the
        reference: it stays until it is replaced or cleared, ``setup`` clears it; no factorization is made for it.  A library without the
        call raises NotImplementedError."""
        self._need('affine')
        if d is None:
            _lib.check(self._L.mpcqp_set_affine(self._h, None, 0), 'mpcqp_set_affine')
            return
        shape = tuple(d.shape)
        per = math.prod(shape[1:]) if len(shape) > 1 and shape[0] == self.batch else math.prod(shape)
        if per not in (self.nx, self.Np * self.nx):
            raise ValueError('d must hold nx or Np*nx values per instance')
        a = _prep(d, (self.batch, per), 'd')
        self._keep = [a]
        _lib.check(self._L.mpcqp_set_affine(self._h, _ptr(a), per // self.nx), 'mpcqp_set_affine')

    def affine_rows(self):
        """Rows of the affine term in force: 0 (none), 1 or Np (mpcqp_get_affine)."""
        self._need('affine')
        rows = C.c_int()
        _lib.check(self._L.mpcqp_get_affine(self._h, None, C.byref(rows)), 'mpcqp_get_affine')
        return rows.value

    def affine(self):
        """The affine term in force [B, rows, nx] (mpcqp_get_affine; synchronises), or None if there is none."""
        rows = self.affine_rows()
        if not rows:
            return None
        d = np.empty((self.batch, rows, self.nx))
        _lib.check(self._L.mpcqp_get_affine(self._h, _ptr(d), C.byref(C.c_int())), 'mpcqp_get_affine')
        return d

    def update_settings(self, **kw):
        kw, polish = _split_polish(kw)
        if polish:
            self._set_polish(**polish)
        for k, v in kw.items():
            if k not in _SETTING_NAMES:
                raise TypeError('unknown solver setting %r' % k)
            if k in _FIXED_AT_CREATE and v != getattr(self.settings, k):
                # (mpcqp_update_settings keeps the handle's own value of these: they shape the problem, the factorization or the kernel choice)
                raise ValueError('solver setting %r is fixed when the problem is created / set up; make a new problem to change it' % k)
            setattr(self.settings, k, v)
        _lib.check(self._L.mpcqp_update_settings(self._h, C.byref(self.settings)), 'mpcqp_update_settings')

    def warm_start(self, x=None, y=None):
        a = _prep(x, (self.batch, self.n), 'x') if x is not None else None
        b = _prep(y, (self.batch, self.m), 'y') if y is not None else None
        _lib.check(self._L.mpcqp_warm_start(self._h, _ptr(a), _ptr(b)), 'mpcqp_warm_start')
        _lib.check(self._L.mpcqp_synchronize(self._h), 'mpcqp_synchronize')

    def solve_async(self):
        _lib.check(self._L.mpcqp_solve(self._h), 'mpcqp_solve')

    def synchronize(self):
        _lib.check(self._L.mpcqp_synchronize(self._h), 'mpcqp_synchronize')

    def mpc_step(self, x0, uminus1=None, xref=None, out=None):
        """One control step ``u = K(x, u_{-1})`` (mpcqp_mpc_step = update + warm solve + output with the u_failure rule)."""
        B, nx, nu = self.batch, self.nx, self.nu
        a = _prep(x0, (B, nx), 'x0')
        b = _prep(uminus1, (B, nu), 'uminus1') if uminus1 is not None else None
        c, rows = None, 1
        if xref is not None:
            rows = self._xref_rows(xref)
            c = _prep(xref, (B, rows * nx), 'xref')
        if out is None:
            out = np.empty((B, nu))
        _lib.check(self._L.mpcqp_mpc_step(self._h, _ptr(a), _ptr(b), _ptr(c), rows, _ptr(out)), 'mpcqp_mpc_step')
        if xref is not None:
            self._xref_rows_last = rows
        return out

    def step_host(self, x0=None, uminus1=None, xref=None):
        """update(x0, uminus1, xref) + warm-started solve + solution in ONE library call with host arrays (mpcqp_step_host):
        the latency path of a single controller.  Returns ``(x [B,n], y [B,m], info[B])`` like ``solution()``."""
        B, nx, nu = self.batch, self.nx, self.nu
        if B == 1 and x0 is not None and uminus1 is not None and xref is not None:
            return self._step_host_one(x0, uminus1, xref)
        f64 = lambda v, cols: v if (type(v) is np.ndarray and v.dtype == np.float64 and v.flags.c_contiguous and v.size == B * cols) \
            else np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(B, cols))      # (a conforming array goes down as it is: same memory, whatever its shape)
        a = None if x0 is None else f64(x0, nx)
        b = None if uminus1 is None else f64(uminus1, nu)
        c, rows = None, 1
        if xref is not None:
            rows = self._xref_rows(xref)
            c = f64(xref, rows * nx)
        x, y = np.empty((B, self.n)), np.empty((B, self.m))
        info = (_lib.Info * B)()
        _lib.check(self._L.mpcqp_step_host(self._h, _ptr(a), _ptr(b), _ptr(c), rows, _ptr(x), _ptr(y), C.cast(info, C.c_void_p)), 'mpcqp_step_host')
        if xref is not None:
            self._xref_rows_last = rows
        return x, y, info

    def _step_host_one(self, x0, uminus1, xref):
        """step_host for ONE controller with the Python side trimmed (a step is ~ 60 us in all: every microsecond here shows): the inputs are
        copied into a buffer the problem keeps -- its three addresses are plain integers computed once -- and x, y come back as views of one
        ctypes block (``ndarray.ctypes.data`` costs ~ 1 us per array, ``np.prod`` of a shape more)."""
        nx, nu, n, m = self.nx, self.nu, self.n, self.m
        hb = self._hin
        if hb is None:
            hb = self._hin = np.empty(nx + nu + (self.Np + 1) * nx)
            p = hb.ctypes.data
            self._hin_p = (p, p + 8 * nx, p + 8 * (nx + nu))
            self._out_t = C.c_double * (n + m)
        xr = xref if type(xref) is np.ndarray else np.asarray(xref, dtype=np.float64)
        nxr = xr.size
        if nxr != nx and nxr != (self.Np + 1) * nx:
            raise ValueError('xref must hold nx or (Np+1)*nx values per instance')
        hb[:nx] = np.reshape(x0, nx); hb[nx:nx + nu] = np.reshape(uminus1, nu); hb[nx + nu:nx + nu + nxr] = xr.reshape(nxr)
        cb = self._out_t()
        info = (_lib.Info * 1)()
        a, b, c = self._hin_p
        _lib.check(self._L.mpcqp_step_host(self._h, a, b, c, nxr // nx, cb, C.addressof(cb) + 8 * n, info), 'mpcqp_step_host')
        self._xref_rows_last = nxr // nx
        buf = np.frombuffer(cb, dtype=np.float64)
        return buf[:n].reshape(1, n), buf[n:].reshape(1, m), info

    def mpc_run(self, nsteps, w=None, Ap=None, Bp=None, out=None, xref_traj=None, estimator=None, model_traj=None, d_traj=None, d_hold=1):
        """Device-side receding-horizon loop (mpcqp_mpc_loop): ``nsteps`` closed-loop steps
        ``u = output(); x = Ap x + Bp u + w[k]; update(x)`` of every instance without host round trips.

        ``w`` [nsteps, batch, nx] (numpy or torch device tensor) or None; ``Ap``/``Bp`` default to the controller model;
        ``xref_traj`` [nsteps, batch, rows*nx] gives the reference of the solve after step k (rows as last uploaded).
        ``estimator = dict(C=[B,ny,nx], L=[B,nx,ny], x_true=[B,nx], v=[nsteps,B,ny] or None)`` switches output feedback on
        (pyMPC/kalman.py:109-134): the controller is updated with the estimate, ``x_true`` is advanced in place.
        ``model_traj = (Ad [nmodels,B,nx,nx] or None, Bd [nmodels,B,nx,nu] or None, hold)`` schedules the model (mpcqp_mpc_loop_tv): entry
        ``k // hold`` replaces Ad / Bd at the start of step k (``update_model``), for the controller and, without ``Ap``/``Bp``, the plant.
        ``d_traj`` [nentries, B, nx] or [nentries, B, Np, nx] schedules the affine term (mpcqp_mpc_loop_affine, include_ext4/mpcqp_affine.h): the solve
        after step k uses entry ``k // d_hold``; the plant does not get the offset (put it into ``w``); the problem is left with the last entry
        used.  Without it a term set with ``set_affine`` stays in force.  Not with an estimator (NotImplementedError).
        Returns ``(x_traj [nsteps+1,B,nx], u_traj [nsteps,B,nu], status [nsteps,B] int32, iters [nsteps,B] int32)`` as
        numpy arrays (plus ``xhat_traj, y_traj`` with an estimator), or fills the arrays/tensors given in ``out``."""
        return self._loop('mpcqp_mpc_loop', nsteps, w=w, Ap=Ap, Bp=Bp, out=out, xref_traj=xref_traj, estimator=estimator, model_traj=model_traj,
                          d_traj=d_traj, d_hold=d_hold)

    def _loop(self, entry, nsteps, w=None, Ap=None, Bp=None, out=None, xref_traj=None, estimator=None, model_traj=None, L_traj=None, d_traj=None, d_hold=1):
        """``mpc_run`` through the C entry point ``entry`` -- mpcqp_mpc_loop, or mpcqp_rollout / mpcqp_rollout_est: the same loop, and a tape
        of it; with a ``model_traj``, mpcqp_mpc_loop_tv (or mpcqp_rollout_tv; mpcqp_mpc_loop_tv_est / mpcqp_rollout_tv_est take an estimator
        and a gain schedule ``L_traj`` too)."""
        K, B, nx, nu = int(nsteps), self.batch, self.nx, self.nu
        io = _lib.Loop()
        keep = []

        def inp(a, shape, name):
            if a is None:
                return None
            a = _prep(a, shape, name); keep.append(a)
            return _ptr(a)

        io.w = inp(w, (K, B, nx), 'w'); io.Ap = inp(Ap, (B, nx, nx), 'Ap'); io.Bp = inp(Bp, (B, nx, nu), 'Bp')
        if xref_traj is not None:
            shp = tuple(xref_traj.shape)
            if B == 1 and len(shp) == 2 and shp[0] == K:          # a single controller's [nsteps, nx] reference sequence
                xref_traj = xref_traj.reshape(K, 1, shp[1]); shp = tuple(xref_traj.shape)
            if len(shp) < 3 or shp[0] != K or shp[1] != B:
                raise ValueError('xref_traj must be [nsteps, batch, nx] or [nsteps, batch, Np+1, nx] (or flattened [nsteps, batch, (Np+1)*nx])')
            per = int(np.prod(shp[2:]))
            if per not in (nx, (self.Np + 1) * nx):
                raise ValueError('xref_traj must hold nx or (Np+1)*nx values per step and instance')
            io.xref_rows = per // nx          # the library checks it again and re-strides its copy accordingly
            io.xref_traj = inp(xref_traj, (K, B, per), 'xref_traj')
        ny = 0
        if estimator is not None:
            Cm = estimator['C']
            ny = int(tuple(Cm.shape)[-2])
            io.ny = ny
            io.C = inp(Cm, (B, ny, nx), 'C'); io.Lgain = inp(estimator.get('L'), (B, nx, ny), 'L')
            io.v = inp(estimator.get('v'), (K, B, ny), 'v')
            xt = estimator['x_true']
            if hasattr(xt, 'ctypes') and not (xt.dtype == np.float64 and xt.flags['C_CONTIGUOUS'] and xt.shape == (B, nx)):
                raise ValueError('estimator["x_true"] must be a C-contiguous float64 [batch, nx] array (it is updated in place)')
            keep.append(xt); io.x_true = _ptr(xt)
        if out is None:
            out = [np.empty((K + 1, B, nx)), np.empty((K, B, nu)), np.empty((K, B), dtype=np.int32), np.empty((K, B), dtype=np.int32)]
            if ny:
                out += [np.empty((K + 1, B, nx)), np.empty((K, B, ny))]
        io.x_traj, io.u_traj, io.status_traj, io.iter_traj = (_ptr(o) for o in out[:4])
        if ny and len(out) >= 6:
            io.xhat_traj, io.y_traj = _ptr(out[4]), _ptr(out[5])
        at = None
        if d_traj is not None:                    # a schedule of affine terms: mpcqp_mpc_loop_affine, with or without a model schedule
            self._need('affine')
            if entry not in ('mpcqp_mpc_loop', 'mpcqp_rollout_affine'):
                raise NotImplementedError('a schedule of affine terms is for mpc_run (mpcqp_mpc_loop_affine): the taped rollouts do not carry the term')
            shp = tuple(d_traj.shape)
            if len(shp) < 3 or shp[1] != B:
                raise ValueError('d_traj must be [nentries, batch, nx] or [nentries, batch, Np, nx]')
            per = int(np.prod(shp[2:]))
            if per not in (nx, self.Np * nx):
                raise ValueError('d_traj must hold nx or Np*nx values per entry and instance')
            at = _lib.AffineTraj()
            at.struct_size, at.hold, at.nentries, at.rows = C.sizeof(_lib.AffineTraj), int(d_hold), int(shp[0]), per // nx
            at.d = inp(d_traj, (shp[0], B, per), 'd_traj')
        if model_traj is not None:
            self._need('model_traj')
            Adt, Bdt, hold = model_traj
            hold = int(hold)
            if hold < 1:
                raise ValueError('model_traj: hold must be >= 1')
            given = [a for a in (Adt, Bdt) if a is not None]
            if not given:
                raise ValueError('model_traj: give Ad, Bd or both')
            nm = int(tuple(given[0].shape)[0])
            mt = _lib.ModelTraj()
            mt.struct_size, mt.hold, mt.nmodels = C.sizeof(_lib.ModelTraj), hold, nm
            mt.Ad = inp(Adt, (nm, B, nx, nx), 'model_traj Ad'); mt.Bd = inp(Bdt, (nm, B, nx, nu), 'model_traj Bd')
            if entry in ('mpcqp_mpc_loop_tv_est', 'mpcqp_rollout_tv_est'):
                et = None
                if L_traj is not None:
                    ne = int(tuple(L_traj.shape)[0])
                    et = _lib.EstTraj()
                    et.struct_size, et.nentries = C.sizeof(_lib.EstTraj), ne
                    et.Lgain_traj = inp(L_traj, (ne, B, nx, ny), 'L_traj')
                rc = getattr(self._L, entry)(self._h, K, C.byref(io), C.byref(mt), None if et is None else C.byref(et))
            elif entry == 'mpcqp_rollout_affine':
                rc = self._L.mpcqp_rollout_affine(self._h, K, C.byref(io), C.byref(mt), None if at is None else C.byref(at))
            elif at is not None:
                entry = 'mpcqp_mpc_loop_affine'
                rc = self._L.mpcqp_mpc_loop_affine(self._h, K, C.byref(io), C.byref(mt), C.byref(at))
            else:
                entry = 'mpcqp_rollout_tv' if entry == 'mpcqp_rollout_tv' else 'mpcqp_mpc_loop_tv'
                rc = getattr(self._L, entry)(self._h, K, C.byref(io), C.byref(mt))
        elif entry == 'mpcqp_rollout_affine':
            rc = self._L.mpcqp_rollout_affine(self._h, K, C.byref(io), None, None if at is None else C.byref(at))
        elif at is not None:
            entry = 'mpcqp_mpc_loop_affine'
            rc = self._L.mpcqp_mpc_loop_affine(self._h, K, C.byref(io), None, C.byref(at))
        else:
            rc = getattr(self._L, entry)(self._h, K, C.byref(io))
        if rc == -4:
            raise NotImplementedError(self._L.mpcqp_last_error().decode())
        _lib.check(rc, entry)
        if xref_traj is not None:
            self._xref_rows_last = int(io.xref_rows)
        self._keep = [keep]                    # (device inputs of a stream-ordered run: alive at least until the next call)
        return tuple(out)

    def solution(self, want_y=True):
        x = np.empty((self.batch, self.n))
        y = np.empty((self.batch, self.m)) if want_y else None
        info = (_lib.Info * self.batch)()
        _lib.check(self._L.mpcqp_get_solution(self._h, _ptr(x), _ptr(y), C.cast(info, C.c_void_p)), 'mpcqp_get_solution')
        return x, y, info

    def infos(self):
        info = (_lib.Info * self.batch)()
        _lib.check(self._L.mpcqp_get_solution(self._h, None, None, C.cast(info, C.c_void_p)), 'mpcqp_get_solution')
        return info

    def u0(self, out=None):
        """First optimal input of every instance, [batch, nu] (numpy, or written into a torch tensor)."""
        if out is None:
            out = np.empty((self.batch, self.nu))
        _lib.check(self._L.mpcqp_get_u0(self._h, _ptr(out)), 'mpcqp_get_u0')
        return out

    def stats(self, reset=False):
        """Cumulative (iterations, residual evaluations, refactorizations, instance-solves) over the batch."""
        out = (C.c_uint64 * 4)()
        _lib.check(self._L.mpcqp_get_stats(self._h, out, int(bool(reset))), 'mpcqp_get_stats')
        return tuple(int(v) for v in out)

    def carry_stats(self):
        """(steps the latency round carried into the next step itself, of those handed back to begin, queue-item parts per instance of the last
        persistent closed-loop launch) -- counters since creation / the last ``stats(reset=True)``."""
        fn = self._L.mpcqp_dev_carry_stats                 # (development export of the HIP library, outside the C ABI)
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        out = (C.c_uint64 * 3)()
        _lib.check(fn(self._h, out), 'mpcqp_dev_carry_stats')
        return tuple(int(v) for v in out)

    def stream_bytes(self):
        """(bytes per ADMM iteration, per round, per solve) one instance streams by design (mpcqp_get_stream_bytes)."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(self._L.mpcqp_get_stream_bytes(self._h, C.byref(a), C.byref(b), C.byref(c)), 'mpcqp_get_stream_bytes')
        return a.value, b.value, c.value

    def mfma_per_iter(self):
        """Matrix-core instructions one instance issues per ADMM iteration (mpcqp_get_work)."""
        v = C.c_int64()
        _lib.check(self._L.mpcqp_get_work(self._h, C.byref(v)), 'mpcqp_get_work')
        return v.value

    def occupancy(self):
        """(workgroups of the solve kernel a compute unit holds, compute units of the device, threads per workgroup) -- mpcqp_get_occupancy."""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        _lib.check(self._L.mpcqp_get_occupancy(self._h, C.byref(a), C.byref(b), C.byref(c)), 'mpcqp_get_occupancy')
        return a.value, b.value, c.value

    def settings_dict(self):
        """The handle's solver settings as a dict (what `update_settings` last sent, on top of what the handle was created with)."""
        return {k: getattr(self.settings, k) for k in _SETTING_NAMES}

    def kernel_name(self, loop):
        buf = C.create_string_buffer(128)
        _lib.check(self._L.mpcqp_kernel_name(self._h, int(bool(loop)), buf, 128), 'mpcqp_kernel_name')
        return buf.value.decode()

    def launch_times(self, nsteps=0):
        """[batch, 2 + nsteps] uint64: entry and exit of every instance's workgroup in the last closed-loop launch and the end of each of its
        first ``nsteps`` (<= 64) steps, ticks of the GPU's 100 MHz clock."""
        out = np.zeros((self.batch, 2 + int(nsteps)), dtype=np.uint64)
        _lib.check(self._L.mpcqp_get_launch_times(self._h, _ptr(out), int(nsteps)), 'mpcqp_get_launch_times')
        return out

    def profile(self, enable=None, reset=False):
        """(milliseconds, launches) of the solve kernel k_mpc_run accumulated while profiling was enabled."""
        ms, nl = C.c_double(), C.c_int64()
        _lib.check(self._L.mpcqp_profile(self._h, -1 if enable is None else int(bool(enable)), C.byref(ms), C.byref(nl), int(bool(reset))), 'mpcqp_profile')
        return ms.value, nl.value

    def status_string(self, code):
        code = int(code)
        if code not in _STATUS_STRINGS:
            _STATUS_STRINGS[code] = self._L.mpcqp_status_string(code).decode()
        return _STATUS_STRINGS[code]

    # -- verification surface -----------------------------------------------------------------
    def export_qp(self):
        B, n, m = self.batch, self.n, self.m
        P, A = np.empty((B, n, n)), np.empty((B, m, n))
        q, l, u = np.empty((B, n)), np.empty((B, m)), np.empty((B, m))
        _lib.check(self._L.mpcqp_export_qp(self._h, _ptr(P), _ptr(A), _ptr(q), _ptr(l), _ptr(u)), 'mpcqp_export_qp')
        return P, q, A, l, u

    def scaling(self):
        D, E = np.empty((self.batch, self.n)), np.empty((self.batch, self.m))
        c, rho = np.empty(self.batch), np.empty(self.batch)
        _lib.check(self._L.mpcqp_get_scaling(self._h, _ptr(D), _ptr(E), _ptr(c), _ptr(rho)), 'mpcqp_get_scaling')
        return D, E, c, rho

    def kkt_solve(self, rhs):
        rhs = _prep(rhs, (self.batch, self.n), 'rhs')
        sol = np.empty((self.batch, self.n))
        _lib.check(self._L.mpcqp_debug_kkt_solve(self._h, _ptr(rhs), _ptr(sol)), 'mpcqp_debug_kkt_solve')
        return sol

    def iterate(self, iters):
        _lib.check(self._L.mpcqp_iterate(self._h, int(iters)), 'mpcqp_iterate')
        self.synchronize()

    def eq_solve(self, sweeps, cold=True, tol=0.0):
        """The equality-constrained part of the QP (dynamics rows only) by at most ``sweeps`` multiplier sweeps with the handle's KKT factor
        (mpcqp_eq_solve); an instance stops once a correction is below ``tol * max(1, |w|)``.  Returns [B, 5]: the four residual norms
        after the last sweep and the sweeps done; the solution is read with ``solution()``."""
        res = np.empty((self.batch, 5))
        _lib.check(self._L.mpcqp_eq_solve(self._h, int(sweeps), int(bool(cold)), float(tol), _ptr(res)), 'mpcqp_eq_solve')
        return res

    def share_factor(self):
        """One model, many states (test_scripts/example_mpc_function.py:105-111): every instance whose factorization inputs are bit-identical to
        instance 0's solves with ONE shared copy of its factor from now on (mpcqp_share_factor) -- call after ``setup`` with the same model and step
        data for every instance, then scatter the states with ``update``.  Results do not change.  Returns the number of instances sharing
        (0 for the register-resident backends)."""
        n = C.c_int(0)
        _lib.check(self._L.mpcqp_share_factor(self._h, C.byref(n)), 'mpcqp_share_factor')
        return int(n.value)

    def refactor(self):
        """Recompute every instance's KKT factor from its current rho (asynchronous; what one rho update costs)."""
        _lib.check(self._L.mpcqp_refactor(self._h), 'mpcqp_refactor')

    def iterate_state(self):
        x, z, y = np.empty((self.batch, self.n)), np.empty((self.batch, self.m)), np.empty((self.batch, self.m))
        _lib.check(self._L.mpcqp_get_iterate(self._h, _ptr(x), _ptr(z), _ptr(y)), 'mpcqp_get_iterate')
        return x, z, y


class DeviceProblem:
    """Single-instance adapter with osqp's call shapes, kept by ``MPCController.prob`` -- and usable in the REFERENCE's own
    class in place of ``osqp.OSQP()`` (mpc.py:241): ``setup(P, q, A, l, u, **settings)``, ``update(q=, l=, u=)``,
    ``solve()`` work on the caller's vectors (the seam of mpc.py:266,454,369).  ``pympc_amd.MPCController`` additionally
    passes ``mpc=`` / ``mpc_step=`` so that the device builds and refreshes q, l, u itself.

    ``nx, nu``: optional hints for reading the controller's dimensions out of P and A (they are inferred otherwise)."""

    def __init__(self, device=0, nx=None, nu=None):
        self.device = device
        self._bp = None
        self._hint = (nx, nu)
        self._model = None
        self._pending = None              # step data of an update() that has not reached the device yet (sent with the solve)

    def _setup_from_matrices(self, P, q, A, l, u, **settings):
        """setup(P, q, A, l, u) of mpc.py:266: the LIBRARY reads the controller out of the matrices and proves it by rebuilding them
        (mpcqp_create_csc / mpcqp_setup_csc, csrc/mpcqp_csc.h); ``NotAnMPCQP`` if they are not pyMPC's."""
        self._bp = BatchProblem.from_matrices(P, A, 1, device=self.device, nx=self._hint[0], nu=self._hint[1], **settings)
        Pc, Ac = self._bp._csc
        one = lambda v: np.asarray(v, dtype=float).reshape(1, -1)
        self._bp.setup_csc(Pc.data[None], Ac.data[None], one(q), one(l), one(u))
        self._model = dict(nx=self._bp.nx, nu=self._bp.nu, Np=self._bp.Np, Nc=self._bp.Nc)
        self.n, self.m = self._bp.n, self._bp.m
        self._model['SOFT_ON'] = self.n > (self._bp.Np + 1) * self._bp.nx + self._bp.Nc * self._bp.nu

    @staticmethod
    def _check_q(mdl, q):
        from . import qp_recover
        nq = (mdl['Np'] + 1) * mdl['nx'] + mdl['Nc'] * mdl['nu']
        q = np.asarray(q, dtype=float)
        if q.shape != (nq + ((mdl['Np'] + 1) * mdl['nx'] if mdl.get('SOFT_ON', True) else 0),) or np.any(q[nq:] != 0.0):
            raise qp_recover.NotAnMPCQP('q must have length n with a zero slack part (mpc.py:599)')

    def setup(self, P=None, q=None, A=None, l=None, u=None, mpc=None, **settings):
        if mpc is None:
            if P is None or q is None or A is None or l is None or u is None:
                raise ValueError('DeviceProblem.setup needs P, q, A, l, u (or the controller data, mpc=...)')
            return self._setup_from_matrices(P, q, A, l, u, **settings)
        xref = np.asarray(mpc['xref'], dtype=float)
        if xref.ndim == 2 and xref.shape[0] != mpc['Np'] + 1:
            raise ValueError('a time-varying xref must have exactly Np+1 rows')
        settings = dict(settings)
        settings.pop('soft_constraints', None)            # (SOFT_ON of the controller is the single source of truth)
        self._bp = BatchProblem(1, mpc['nx'], mpc['nu'], mpc['Np'], mpc['Nc'], device=self.device,
                                soft_constraints=int(bool(mpc.get('SOFT_ON', True))), **settings)
        one = lambda a: np.asarray(a, dtype=float)[None]
        self._bp.setup(one(mpc['Ad']), one(mpc['Bd']), one(mpc['Qx']), one(mpc['QxN']), one(mpc['Qu']), one(mpc['QDu']),
                       one(mpc['xmin']), one(mpc['xmax']), one(mpc['umin']), one(mpc['umax']),
                       one(mpc['Dumin']), one(mpc['Dumax']), one(mpc['uref']), np.array([[mpc['eps_feas']]]),
                       one(mpc['x0']), one(mpc['uminus1']), xref.reshape(1, -1))
        self.n, self.m = self._bp.n, self._bp.m

    def flush(self):
        """Send the step data of the last update() to the device now (it otherwise travels with the solve that follows)."""
        if self._pending is not None:
            pend, self._pending = self._pending, None
            self._bp.update(*pend)

    def update(self, q=None, l=None, u=None, mpc_step=None, **unsupported):
        if unsupported:
            raise NotImplementedError('DeviceProblem.update supports q, l, u (what pyMPC updates, mpc.py:454); got %s' % sorted(unsupported))
        if mpc_step is None:                              # the caller's vectors, verbatim
            self.flush()
            if self._model is None:
                from . import qp_recover
                raise qp_recover.NotAnMPCQP('update(q=, l=, u=) needs a problem set up from P, q, A, l, u')
            from . import qp_recover
            qp_recover.check_vectors(self._model, l, u)
            if q is not None:
                self._check_q(self._model, q)
            clip = lambda v: None if v is None else np.clip(np.asarray(v, dtype=float), -1e30, 1e30)[None]
            self._bp.update_vectors(None if q is None else np.asarray(q, dtype=float)[None], clip(l), clip(u))
            return
        # kept on the host until the solve that follows (mpc.py:338-364: update() = refresh + solve): one library call, one launch
        if isinstance(mpc_step, tuple):                   # (x0, uminus1, xref) as private float64 copies: MPCController's snapshot
            self._pending = mpc_step
        else:
            self._pending = (np.array(mpc_step['x0'], dtype=float).reshape(1, -1), np.array(mpc_step['uminus1'], dtype=float).reshape(1, -1),
                             np.array(mpc_step['xref'], dtype=float).reshape(1, -1))

    def update_settings(self, **kw):
        self._bp.update_settings(**kw)

    @property
    def supports_update_model(self):
        """True if the loaded solver library has mpcqp_update_model (include/mpcqp_model.h)."""
        return _lib.has_model_update()

    def update_model(self, **fields):
        """New controller data under the problem in use (``BatchProblem.update_model`` for the one instance): Ad, Bd, Qx, QxN, Qu, QDu, xmin, xmax,
        umin, umax, Dumin, Dumax, uref, eps_feas -- None or absent = unchanged.  The iterate is kept; the next ``solve()`` warm-starts from it."""
        self.flush()
        one = lambda k, v: np.array([[float(v)]]) if k == 'eps_feas' else np.asarray(v, dtype=float)[None]
        self._bp.update_model(**{k: one(k, v) for k, v in fields.items() if v is not None})

    def set_affine(self, d):
        """The affine term of the prediction model for the one instance (``BatchProblem.set_affine``): [nx], [Np, nx] or None (clear)."""
        self.flush()
        self._bp.set_affine(None if d is None else np.asarray(d, dtype=float).reshape(1, -1))

    def warm_start(self, x=None, y=None):
        self.flush()
        self._bp.warm_start(None if x is None else np.asarray(x)[None], None if y is None else np.asarray(y)[None])

    def solve(self):
        if self._pending is not None:
            pend, self._pending = self._pending, None
            x, y, info = self._bp.step_host(*pend)
        else:
            self._bp.solve_async()
            x, y, info = self._bp.solution()
        res = Result(x[0], y[0], info[0], self._bp.status_string(info[0].status))
        if self._bp.polishing:
            res.info.status_polish = int(self._bp.polish_status()[0])
        return res

    @property
    def batch_problem(self):
        self.flush()
        return self._bp
