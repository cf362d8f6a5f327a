"""ctypes binding of libmpcqp_hip.so (C ABI declared in include/mpcqp.h).

There is deliberately no fallback: if the shared library has not been built
(``python -c 'import __graft_entry__ as g; g.build()'`` or ``pympc_amd/csrc/build.sh``)
loading raises, and creating a problem without a GPU raises ``RuntimeError``.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libmpcqp_hip.so')     # the in-tree build, nothing else (no environment override)

# every symbol declared in include/mpcqp.h
SYMBOLS = [
    'mpcqp_default_settings', 'mpcqp_status_string', 'mpcqp_last_error', 'mpcqp_device_count',
    'mpcqp_create', 'mpcqp_destroy', 'mpcqp_set_stream', 'mpcqp_synchronize',
    'mpcqp_setup', 'mpcqp_setup_qp', 'mpcqp_create_csc', 'mpcqp_setup_csc', 'mpcqp_update', 'mpcqp_update_vectors', 'mpcqp_warm_start', 'mpcqp_update_settings', 'mpcqp_solve',
    'mpcqp_mpc_step', 'mpcqp_step_host', 'mpcqp_mpc_run', 'mpcqp_mpc_loop', 'mpcqp_get_solution', 'mpcqp_get_u0', 'mpcqp_get_shape', 'mpcqp_get_dims', 'mpcqp_get_stream_bytes', 'mpcqp_get_work', 'mpcqp_get_occupancy', 'mpcqp_kernel_name', 'mpcqp_get_stats', 'mpcqp_get_launch_times', 'mpcqp_profile',
    'mpcqp_export_qp', 'mpcqp_get_scaling', 'mpcqp_debug_kkt_solve', 'mpcqp_get_iterate', 'mpcqp_iterate', 'mpcqp_refactor', 'mpcqp_share_factor', 'mpcqp_eq_solve',
]

# include/mpcqp_polish.h: an extension beside mpcqp.h, bound only where the loaded library exports it (the CPU twin does not)
POLISH_SYMBOLS = ['mpcqp_polish_default_settings', 'mpcqp_set_polish', 'mpcqp_polish', 'mpcqp_get_polish_info']

# include/mpcqp_model.h: likewise -- a new model under a handle that is in use, and a schedule of models for the device loop
MODEL_SYMBOLS = ['mpcqp_update_model', 'mpcqp_mpc_loop_tv']

# include/mpcqp_adjoint.h: likewise -- adjoint derivatives of the solution and the gains of the constrained control law
ADJOINT_SYMBOLS = ['mpcqp_adjoint_default_settings', 'mpcqp_set_adjoint', 'mpcqp_adjoint', 'mpcqp_gains', 'mpcqp_get_adjoint_info']

# include/mpcqp_adjoint_model.h: likewise -- the matrix half of the adjoint: gradients for Ad, Bd, Qx, QxN, Qu, QDu, eps_feas
ADJOINT_MODEL_SYMBOLS = ['mpcqp_adjoint_model']
ADJOINT_MODEL_NAMES = ('Ad', 'Bd', 'Qx', 'QxN', 'Qu', 'QDu', 'eps_feas')      # the outputs of mpcqp_adjoint_model_io, in its order

# include/mpcqp_rollout.h: likewise -- the device loop with a tape, and its derivative in one reverse sweep
ROLLOUT_SYMBOLS = ['mpcqp_rollout', 'mpcqp_rollout_tape_bytes', 'mpcqp_rollout_release', 'mpcqp_rollout_adjoint', 'mpcqp_get_rollout_info',
                   'mpcqp_rollout_get_tape']

# include/mpcqp_rollout_est.h: likewise -- the taped rollout of the output-feedback loop, differentiated through the estimator
ROLLOUT_EST_SYMBOLS = ['mpcqp_rollout_est', 'mpcqp_rollout_est_tape_bytes', 'mpcqp_rollout_adjoint_est', 'mpcqp_rollout_get_tape_est']

# include/mpcqp_adjoint_bounds.h: likewise -- the adjoint chained into the constraint bounds, for the single solve and for the sweeps
ADJOINT_BOUNDS_SYMBOLS = ['mpcqp_adjoint_bounds', 'mpcqp_rollout_adjoint_bounds']
ADJOINT_BOUNDS_NAMES = ('xmin', 'xmax', 'umin', 'umax', 'Dumin', 'Dumax')      # the outputs of mpcqp_adjoint_bounds_io, in its order

# include_ext/mpcqp_rollout_tv.h: likewise -- the taped rollout under a model schedule, and its reverse sweep with per-slot model gradients
ROLLOUT_TV_SYMBOLS = ['mpcqp_rollout_tv', 'mpcqp_rollout_tv_tape_bytes', 'mpcqp_rollout_adjoint_tv', 'mpcqp_rollout_tv_get_slot']

# include_ext2/mpcqp_rollout_tv_est.h: likewise -- the output-feedback loop under a model (and gain) schedule, its tape and its reverse sweep
ROLLOUT_TV_EST_SYMBOLS = ['mpcqp_mpc_loop_tv_est', 'mpcqp_rollout_tv_est', 'mpcqp_rollout_tv_est_tape_bytes', 'mpcqp_rollout_adjoint_tv_est',
                          'mpcqp_rollout_tv_est_get_gain']

# include/mpcqp_riccati.h: likewise -- batched discrete algebraic Riccati equations and their adjoint, without a handle
RICCATI_SYMBOLS = ['mpcqp_riccati_default_settings', 'mpcqp_dare', 'mpcqp_dare_adjoint']

# include_ext3/mpcqp_riccati_traj.h: likewise -- batched Riccati difference equations (a recursion over a model trajectory) and their adjoint
RICCATI_TRAJ_SYMBOLS = ['mpcqp_dre', 'mpcqp_dre_adjoint']

# include_ext4/mpcqp_affine.h: likewise -- an affine term d in the prediction model x+ = Ad x + Bd u + d, its schedule in the device loop and its gradient
AFFINE_SYMBOLS = ['mpcqp_set_affine', 'mpcqp_get_affine', 'mpcqp_mpc_loop_affine', 'mpcqp_adjoint_affine']

# include_ext5/mpcqp_rollout_affine.h: likewise -- the taped rollout with an affine term (constant or scheduled, with or without a model schedule) and its
# reverse sweep with the gradient of every term
ROLLOUT_AFFINE_SYMBOLS = ['mpcqp_rollout_affine', 'mpcqp_rollout_affine_tape_bytes', 'mpcqp_rollout_adjoint_affine', 'mpcqp_rollout_affine_get_slot',
                          'mpcqp_rollout_affine_get_tape', 'mpcqp_gains_affine']


class RiccatiSettings(C.Structure):
    """mpcqp_riccati_settings (include/mpcqp_riccati.h)."""
    _fields_ = [('struct_size', C.c_int32), ('max_iter', C.c_int32), ('gain_form', C.c_int32), ('reserved', C.c_int32), ('tol', C.c_double)]


class PolishSettings(C.Structure):
    """mpcqp_polish_settings (include/mpcqp_polish.h)."""
    _fields_ = [('struct_size', C.c_int32), ('polish', C.c_int32), ('delta', C.c_double),
                ('polish_refine_iter', C.c_int32), ('reserved', C.c_int32)]


class AdjointSettings(C.Structure):
    """mpcqp_adjoint_settings (include/mpcqp_adjoint.h)."""
    _fields_ = [('struct_size', C.c_int32), ('refine_iter', C.c_int32), ('delta', C.c_double), ('weak_tol', C.c_double),
                ('extra_iter', C.c_int32), ('reserved', C.c_int32)]


class AdjointIO(C.Structure):
    """mpcqp_adjoint_io (include/mpcqp_adjoint.h): seeds in, gradients out; host or device pointers, None = not given / not wanted."""
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('g_w', C.c_void_p), ('g_u0', C.c_void_p),
                ('d_x0', C.c_void_p), ('d_uminus1', C.c_void_p), ('d_xref', C.c_void_p), ('d_uref', C.c_void_p),
                ('d_q', C.c_void_p), ('d_l', C.c_void_p), ('d_u', C.c_void_p)]


class AdjointModelIO(C.Structure):
    """mpcqp_adjoint_model_io (include/mpcqp_adjoint_model.h): model gradients out; host or device pointers, None = not wanted."""
    _fields_ = [('struct_size', C.c_int32), ('batch_sum', C.c_int32), ('d_Ad', C.c_void_p), ('d_Bd', C.c_void_p), ('d_Qx', C.c_void_p),
                ('d_QxN', C.c_void_p), ('d_Qu', C.c_void_p), ('d_QDu', C.c_void_p), ('d_eps_feas', C.c_void_p)]


class AdjointBoundsIO(C.Structure):
    """mpcqp_adjoint_bounds_io (include/mpcqp_adjoint_bounds.h): bound gradients out; host or device pointers, None = not wanted."""
    _fields_ = [('struct_size', C.c_int32), ('batch_sum', C.c_int32), ('d_xmin', C.c_void_p), ('d_xmax', C.c_void_p), ('d_umin', C.c_void_p),
                ('d_umax', C.c_void_p), ('d_Dumin', C.c_void_p), ('d_Dumax', C.c_void_p)]


class RolloutAdjointIO(C.Structure):
    """mpcqp_rollout_adjoint_io (include/mpcqp_rollout.h): trajectory seeds in, gradients out; host or device pointers, None = not given / not wanted."""
    _fields_ = [('struct_size', C.c_int32), ('no_reuse', C.c_int32), ('G_x', C.c_void_p), ('G_u', C.c_void_p),
                ('lam', C.c_void_p), ('d_uminus1', C.c_void_p), ('d_uref', C.c_void_p), ('d_xref', C.c_void_p),
                ('d_Ap', C.c_void_p), ('d_Bp', C.c_void_p)]


class RolloutEstIO(C.Structure):
    """mpcqp_rollout_est_io (include/mpcqp_rollout_est.h): the estimator's seeds in, gradients out; host or device pointers, None = not given / not wanted."""
    _fields_ = [('struct_size', C.c_int32), ('G_xhat', C.c_void_p), ('G_y', C.c_void_p), ('eta', C.c_void_p), ('d_C', C.c_void_p),
                ('d_L', C.c_void_p), ('d_v', C.c_void_p), ('d_Ae', C.c_void_p), ('d_Be', C.c_void_p)]


class RolloutTVIO(C.Structure):
    """mpcqp_rollout_tv_io (include_ext/mpcqp_rollout_tv.h): the per-slot and per-entry model gradients out; host or device pointers, None = not wanted."""
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('d_Ad_slots', C.c_void_p), ('d_Bd_slots', C.c_void_p),
                ('d_Ap_entries', C.c_void_p), ('d_Bp_entries', C.c_void_p)]


class EstTraj(C.Structure):
    """mpcqp_est_traj (include_ext2/mpcqp_rollout_tv_est.h): entry e of Lgain_traj is the observer gain while model entry e is in force."""
    _fields_ = [('struct_size', C.c_int32), ('nentries', C.c_int32), ('Lgain_traj', C.c_void_p)]


class RolloutTVEstIO(C.Structure):
    """mpcqp_rollout_tv_est_io (include_ext2/mpcqp_rollout_tv_est.h): the per-entry estimator gradients out; host or device pointers, None = not wanted."""
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('d_Ae_entries', C.c_void_p), ('d_Be_entries', C.c_void_p),
                ('d_L_entries', C.c_void_p)]


class Settings(C.Structure):
    _fields_ = [('rho', C.c_double), ('sigma', C.c_double), ('alpha', C.c_double),
                ('eps_abs', C.c_double), ('eps_rel', C.c_double),
                ('eps_prim_inf', C.c_double), ('eps_dual_inf', C.c_double),
                ('adaptive_rho_tolerance', C.c_double),
                ('max_iter', C.c_int32), ('check_termination', C.c_int32), ('scaling', C.c_int32),
                ('adaptive_rho', C.c_int32), ('adaptive_rho_interval', C.c_int32), ('warm_start', C.c_int32),
                ('soft_constraints', C.c_int32), ('backend', C.c_int32), ('tuning', C.c_int32)]


# enum mpcqp_backend / mpcqp_tuning of include/mpcqp.h
BACKEND_AUTO, BACKEND_SWEEPS, BACKEND_DENSE, BACKEND_BCR, BACKEND_BCR8, BACKEND_BCRT = 0, 1, 2, 3, 4, 5
TUNE_NO_BALANCE, TUNE_NO_LSTAGE, TUNE_NO_GROUPING, TUNE_NO_W8, TUNE_NO_QUEUE, TUNE_NO_PARTS = 1, 2, 4, 8, 16, 32
TUNE_NO_SHARE = 1 << 30    # every instance keeps to its own factor (mpcqp_share_factor)
TUNE_ITEMS_SHIFT = 16      # development: tuning bits 16..22 = queue items per resident slot of a persistent closed-loop launch (include/mpcqp.h)
TUNE_NO_CARRY = 1 << 23    # development: the device loop leaves the latency round after every solve (A/B switch: results are the same)
TUNE_PACE_SHIFT = 8        # development: tuning bits 8..15 = pacing units (include/mpcqp.h)


class Info(C.Structure):
    _fields_ = [('status', C.c_int32), ('iter', C.c_int32), ('rho_updates', C.c_int32), ('reserved', C.c_int32),
                ('obj_val', C.c_double), ('pri_res', C.c_double), ('dua_res', C.c_double), ('rho', C.c_double)]


_pd = C.POINTER(C.c_double)


class Model(C.Structure):
    _fields_ = [(k, _pd) for k in ('Ad', 'Bd', 'Qx', 'QxN', 'Qu', 'QDu', 'xmin', 'xmax', 'umin', 'umax',
                                   'Dumin', 'Dumax', 'uref', 'eps_feas')]


class Loop(C.Structure):
    """mpcqp_loop (include/mpcqp.h): optional inputs/outputs of the device-side closed loop."""
    _fields_ = [('w', C.c_void_p), ('Ap', C.c_void_p), ('Bp', C.c_void_p), ('xref_traj', C.c_void_p),
                ('ny', C.c_int32), ('xref_rows', C.c_int32),
                ('C', C.c_void_p), ('Lgain', C.c_void_p), ('v', C.c_void_p), ('x_true', C.c_void_p),
                ('x_traj', C.c_void_p), ('xhat_traj', C.c_void_p), ('y_traj', C.c_void_p), ('u_traj', C.c_void_p),
                ('status_traj', C.c_void_p), ('iter_traj', C.c_void_p)]


class ModelTraj(C.Structure):
    """mpcqp_model_traj (include/mpcqp_model.h): entry e of Ad / Bd is in force during steps e * hold .. e * hold + hold - 1."""
    _fields_ = [('struct_size', C.c_int32), ('hold', C.c_int32), ('nmodels', C.c_int32), ('reserved', C.c_int32),
                ('Ad', C.c_void_p), ('Bd', C.c_void_p)]


class AffineTraj(C.Structure):
    """mpcqp_affine_traj (include_ext4/mpcqp_affine.h): entry e of d is the affine term of the solves after steps e * hold .. e * hold + hold - 1."""
    _fields_ = [('struct_size', C.c_int32), ('hold', C.c_int32), ('nentries', C.c_int32), ('rows', C.c_int32), ('d', C.c_void_p)]


class RolloutAffineIO(C.Structure):
    """mpcqp_rollout_affine_io (include_ext5/mpcqp_rollout_affine.h): the gradient of the affine terms per slot out; a host or device pointer, None = not wanted."""
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('d_d_slots', C.c_void_p)]


_lib = None


def load():
    """Load the HIP library (once) and declare the prototypes of include/mpcqp.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libmpcqp_hip.so is missing (%s). Build it with pympc_amd/csrc/build.sh; "
            "pympc_amd has no CPU fallback." % LIB_PATH)
    # One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64 / libhsa-runtime64 with the same sonames as /opt/rocm's, so
    # whichever is mapped first serves both: this library works on top of torch's, torch on top of the system's reports "No HIP GPUs are
    # available" at its first CUDA call.  Where torch is installed it therefore loads first (it is the package's plumbing for device
    # buffers, streams and torch.distributed anyway).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    H = C.c_void_p
    L.mpcqp_default_settings.argtypes = [C.POINTER(Settings)]
    L.mpcqp_default_settings.restype = None
    L.mpcqp_status_string.argtypes = [C.c_int]
    L.mpcqp_status_string.restype = C.c_char_p
    L.mpcqp_last_error.restype = C.c_char_p
    L.mpcqp_device_count.restype = C.c_int
    L.mpcqp_create.argtypes = [C.POINTER(H), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Settings)]
    L.mpcqp_destroy.argtypes = [H]
    L.mpcqp_destroy.restype = None
    L.mpcqp_set_stream.argtypes = [H, C.c_void_p]
    L.mpcqp_synchronize.argtypes = [H]
    L.mpcqp_setup.argtypes = [H, C.POINTER(Model), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.mpcqp_update.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.mpcqp_setup_qp.argtypes = [H, C.POINTER(Model), C.c_void_p, C.c_void_p, C.c_void_p]
    L.mpcqp_update_vectors.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mpcqp_create_csc.argtypes = [C.POINTER(H), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(Settings)]
    L.mpcqp_setup_csc.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mpcqp_warm_start.argtypes = [H, C.c_void_p, C.c_void_p]
    L.mpcqp_update_settings.argtypes = [H, C.POINTER(Settings)]
    L.mpcqp_solve.argtypes = [H]
    L.mpcqp_mpc_run.argtypes = [H, C.c_int] + [C.c_void_p] * 7
    L.mpcqp_mpc_step.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.mpcqp_mpc_loop.argtypes = [H, C.c_int, C.POINTER(Loop)]
    L.mpcqp_step_host.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mpcqp_get_solution.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mpcqp_get_u0.argtypes = [H, C.c_void_p]
    L.mpcqp_get_shape.argtypes = [H] + [C.POINTER(C.c_int)] * 4
    L.mpcqp_get_dims.argtypes = [H, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.mpcqp_get_stream_bytes.argtypes = [H, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.mpcqp_get_work.argtypes = [H, C.POINTER(C.c_int64)]
    L.mpcqp_get_occupancy.argtypes = [H] + [C.POINTER(C.c_int)] * 3
    L.mpcqp_kernel_name.argtypes = [H, C.c_int, C.c_char_p, C.c_int]
    L.mpcqp_get_stats.argtypes = [H, C.POINTER(C.c_uint64), C.c_int]
    L.mpcqp_get_launch_times.argtypes = [H, C.c_void_p, C.c_int]
    L.mpcqp_profile.argtypes = [H, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]
    L.mpcqp_export_qp.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mpcqp_get_scaling.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mpcqp_debug_kkt_solve.argtypes = [H, C.c_void_p, C.c_void_p]
    L.mpcqp_get_iterate.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mpcqp_iterate.argtypes = [H, C.c_int]
    L.mpcqp_refactor.argtypes = [H]
    L.mpcqp_share_factor.argtypes = [H, C.POINTER(C.c_int)]
    L.mpcqp_eq_solve.argtypes = [H, C.c_int, C.c_int, C.c_double, C.c_void_p]
    for name in SYMBOLS:
        getattr(L, name)           # AttributeError here = header and library out of sync
        if name not in ('mpcqp_default_settings', 'mpcqp_status_string', 'mpcqp_last_error', 'mpcqp_destroy'):
            getattr(L, name).restype = C.c_int
    if has_polish(L):
        L.mpcqp_polish_default_settings.argtypes = [C.POINTER(PolishSettings)]
        L.mpcqp_polish_default_settings.restype = None
        L.mpcqp_set_polish.argtypes = [H, C.POINTER(PolishSettings)]
        L.mpcqp_polish.argtypes = [H]
        L.mpcqp_get_polish_info.argtypes = [H, C.c_void_p]
        for name in ('mpcqp_set_polish', 'mpcqp_polish', 'mpcqp_get_polish_info'):
            getattr(L, name).restype = C.c_int
    if has_model_update(L):
        L.mpcqp_update_model.argtypes = [H, C.POINTER(Model)]
        L.mpcqp_mpc_loop_tv.argtypes = [H, C.c_int, C.POINTER(Loop), C.POINTER(ModelTraj)]
        for name in MODEL_SYMBOLS:
            getattr(L, name).restype = C.c_int
    if has_adjoint(L):
        L.mpcqp_adjoint_default_settings.argtypes = [C.POINTER(AdjointSettings)]
        L.mpcqp_adjoint_default_settings.restype = None
        L.mpcqp_set_adjoint.argtypes = [H, C.POINTER(AdjointSettings)]
        L.mpcqp_adjoint.argtypes = [H, C.POINTER(AdjointIO)]
        L.mpcqp_gains.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mpcqp_get_adjoint_info.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ADJOINT_SYMBOLS[1:]:
            getattr(L, name).restype = C.c_int
    if has_adjoint_model(L):
        L.mpcqp_adjoint_model.argtypes = [H, C.POINTER(AdjointIO), C.POINTER(AdjointModelIO)]
        L.mpcqp_adjoint_model.restype = C.c_int
    if has_rollout(L):
        L.mpcqp_rollout.argtypes = [H, C.c_int, C.POINTER(Loop)]
        L.mpcqp_rollout_tape_bytes.argtypes = [H, C.c_int, C.POINTER(C.c_int64)]
        L.mpcqp_rollout_release.argtypes = [H]
        L.mpcqp_rollout_adjoint.argtypes = [H, C.POINTER(RolloutAdjointIO), C.POINTER(AdjointModelIO)]
        L.mpcqp_get_rollout_info.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mpcqp_rollout_get_tape.argtypes = [H, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ROLLOUT_SYMBOLS:
            getattr(L, name).restype = C.c_int
    if has_rollout_est(L):
        L.mpcqp_rollout_est.argtypes = [H, C.c_int, C.POINTER(Loop)]
        L.mpcqp_rollout_est_tape_bytes.argtypes = [H, C.c_int, C.c_int, C.POINTER(C.c_int64)]
        L.mpcqp_rollout_adjoint_est.argtypes = [H, C.POINTER(RolloutAdjointIO), C.POINTER(RolloutEstIO), C.POINTER(AdjointModelIO)]
        L.mpcqp_rollout_get_tape_est.argtypes = [H, C.c_int, C.c_void_p, C.c_void_p]
        for name in ROLLOUT_EST_SYMBOLS:
            getattr(L, name).restype = C.c_int
    if has_adjoint_bounds(L):
        L.mpcqp_adjoint_bounds.argtypes = [H, C.POINTER(AdjointIO), C.POINTER(AdjointModelIO), C.POINTER(AdjointBoundsIO)]
        L.mpcqp_rollout_adjoint_bounds.argtypes = [H, C.POINTER(RolloutAdjointIO), C.POINTER(RolloutEstIO), C.POINTER(AdjointModelIO), C.POINTER(AdjointBoundsIO)]
        for name in ADJOINT_BOUNDS_SYMBOLS:
            getattr(L, name).restype = C.c_int
    if has_rollout_tv(L):
        L.mpcqp_rollout_tv.argtypes = [H, C.c_int, C.POINTER(Loop), C.POINTER(ModelTraj)]
        L.mpcqp_rollout_tv_tape_bytes.argtypes = [H, C.c_int, C.c_int, C.POINTER(C.c_int64)]
        L.mpcqp_rollout_adjoint_tv.argtypes = [H, C.POINTER(RolloutAdjointIO), C.POINTER(AdjointModelIO), C.POINTER(AdjointBoundsIO), C.POINTER(RolloutTVIO)]
        L.mpcqp_rollout_tv_get_slot.argtypes = [H, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ROLLOUT_TV_SYMBOLS:
            getattr(L, name).restype = C.c_int
    if has_rollout_tv_est(L):
        L.mpcqp_mpc_loop_tv_est.argtypes = [H, C.c_int, C.POINTER(Loop), C.POINTER(ModelTraj), C.POINTER(EstTraj)]
        L.mpcqp_rollout_tv_est.argtypes = [H, C.c_int, C.POINTER(Loop), C.POINTER(ModelTraj), C.POINTER(EstTraj)]
        L.mpcqp_rollout_tv_est_tape_bytes.argtypes = [H, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]
        L.mpcqp_rollout_adjoint_tv_est.argtypes = [H, C.POINTER(RolloutAdjointIO), C.POINTER(RolloutEstIO), C.POINTER(AdjointModelIO), C.POINTER(AdjointBoundsIO),
                                                   C.POINTER(RolloutTVIO), C.POINTER(RolloutTVEstIO)]
        L.mpcqp_rollout_tv_est_get_gain.argtypes = [H, C.c_int, C.c_void_p]
        for name in ROLLOUT_TV_EST_SYMBOLS:
            getattr(L, name).restype = C.c_int
    if has_riccati(L):
        L.mpcqp_riccati_default_settings.argtypes = [C.POINTER(RiccatiSettings)]
        L.mpcqp_riccati_default_settings.restype = None
        L.mpcqp_dare.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(RiccatiSettings)] + [C.c_void_p] * 9
        L.mpcqp_dare_adjoint.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(RiccatiSettings)] + [C.c_void_p] * 14
        for name in RICCATI_SYMBOLS[1:]:
            getattr(L, name).restype = C.c_int
    if has_riccati_traj(L):
        head = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(RiccatiSettings), C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.mpcqp_dre.argtypes = head + [C.c_void_p] * 7
        L.mpcqp_dre_adjoint.argtypes = head + [C.c_void_p] * 12
        for name in RICCATI_TRAJ_SYMBOLS:
            getattr(L, name).restype = C.c_int
    if has_affine(L):
        L.mpcqp_set_affine.argtypes = [H, C.c_void_p, C.c_int]
        L.mpcqp_get_affine.argtypes = [H, C.c_void_p, C.POINTER(C.c_int)]
        L.mpcqp_mpc_loop_affine.argtypes = [H, C.c_int, C.POINTER(Loop), C.POINTER(ModelTraj), C.POINTER(AffineTraj)]
        L.mpcqp_adjoint_affine.argtypes = [H, C.POINTER(AdjointIO), C.c_void_p]
        for name in AFFINE_SYMBOLS:
            getattr(L, name).restype = C.c_int
    if has_rollout_affine(L):
        L.mpcqp_rollout_affine.argtypes = [H, C.c_int, C.POINTER(Loop), C.POINTER(ModelTraj), C.POINTER(AffineTraj)]
        L.mpcqp_rollout_affine_tape_bytes.argtypes = [H, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]
        L.mpcqp_rollout_adjoint_affine.argtypes = [H, C.POINTER(RolloutAdjointIO), C.POINTER(AdjointModelIO), C.POINTER(AdjointBoundsIO), C.POINTER(RolloutTVIO),
                                                   C.POINTER(RolloutAffineIO)]
        L.mpcqp_rollout_affine_get_slot.argtypes = [H, C.c_int, C.c_void_p]
        L.mpcqp_rollout_affine_get_tape.argtypes = [H, C.c_int, C.c_void_p]
        L.mpcqp_gains_affine.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ROLLOUT_AFFINE_SYMBOLS:
            getattr(L, name).restype = C.c_int
    _lib = L
    return L


def _has(L, symbols):
    """True if the library (None: the loaded one) exports every one of ``symbols``: libmpcqp_hip.so does, the CPU twin does not."""
    L = L if L is not None else load()
    return all(hasattr(L, name) for name in symbols)


def has_polish(L=None):
    """True if the library exports include/mpcqp_polish.h."""
    return _has(L, POLISH_SYMBOLS)


def has_model_update(L=None):
    """True if the library exports include/mpcqp_model.h."""
    return _has(L, MODEL_SYMBOLS)


def has_adjoint(L=None):
    """True if the library exports include/mpcqp_adjoint.h."""
    return _has(L, ADJOINT_SYMBOLS)


def has_adjoint_model(L=None):
    """True if the library exports include/mpcqp_adjoint_model.h."""
    return _has(L, ADJOINT_MODEL_SYMBOLS)


def has_rollout(L=None):
    """True if the library exports include/mpcqp_rollout.h."""
    return _has(L, ROLLOUT_SYMBOLS)


def has_rollout_est(L=None):
    """True if the library exports include/mpcqp_rollout_est.h."""
    return _has(L, ROLLOUT_EST_SYMBOLS)


def has_adjoint_bounds(L=None):
    """True if the library exports include/mpcqp_adjoint_bounds.h."""
    return _has(L, ADJOINT_BOUNDS_SYMBOLS)


def has_rollout_tv(L=None):
    """True if the library exports include_ext/mpcqp_rollout_tv.h."""
    return _has(L, ROLLOUT_TV_SYMBOLS)


def has_rollout_tv_est(L=None):
    """True if the library exports include_ext2/mpcqp_rollout_tv_est.h."""
    return _has(L, ROLLOUT_TV_EST_SYMBOLS)


def has_riccati(L=None):
    """True if the library exports include/mpcqp_riccati.h."""
    return _has(L, RICCATI_SYMBOLS)


def has_riccati_traj(L=None):
    """True if the library exports include_ext3/mpcqp_riccati_traj.h."""
    return _has(L, RICCATI_TRAJ_SYMBOLS)


def has_affine(L=None):
    """True if the library exports include_ext4/mpcqp_affine.h."""
    return _has(L, AFFINE_SYMBOLS)


def has_rollout_affine(L=None):
    """True if the library exports include_ext5/mpcqp_rollout_affine.h."""
    return _has(L, ROLLOUT_AFFINE_SYMBOLS)


def check(rc, what):
    if rc != 0:
        msg = load().mpcqp_last_error().decode()
        raise RuntimeError('%s failed (%d): %s' % (what, rc, msg))
