"""include_ext2/mpcqp_rollout_tv_est.h -- the output-feedback loop under a model schedule, its tape and its reverse sweep, in a directory
of its own beside include/ and include_ext/: exported by the HIP library, bound by pympc_amd._lib in a symbol list of its own, its structs
mirrored field by field, include/ and include_ext/ untouched; a library without it (the CPU twin) makes the Python methods raise
NotImplementedError and leaves the controller where it was.  No GPU needed."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from util import repeated
from abi import (ROOT, header_struct, ctypes_struct, header_functions, lib_loaded, OLDER_HEADERS, ADJOINT_HEADER_SHA256,
                 ADJOINT_MODEL_HEADER_SHA256, twin)      # noqa: F401  (twin: a fixture)

HEADER = open(os.path.join(ROOT, 'include_ext2', 'mpcqp_rollout_tv_est.h')).read()
FUNCTIONS = ['mpcqp_mpc_loop_tv_est', 'mpcqp_rollout_adjoint_tv_est', 'mpcqp_rollout_tv_est', 'mpcqp_rollout_tv_est_get_gain', 'mpcqp_rollout_tv_est_tape_bytes']
# include/ and include_ext/ as this extension found them (sha256 of the files that came after tests/abi.py's)
NEWER_HEADERS = {
    'mpcqp_rollout.h': 'b77eed88f091515afe45b3d05f1a4f24fd6a15d507578c3a0892371e6e55f978',
    'mpcqp_rollout_est.h': 'bdceeaa9c89cb16b1c95a9fbe8f60c04d1a7fb72cbf675f9b3529beaca3f142d',
    'mpcqp_riccati.h': '9a711292b530a9700c4c96e5520ae7ed296b77044e82876778c817f79e9fe6a2',
    'mpcqp_adjoint_bounds.h': 'e059764945990e3cc234a8f3a959b8cda17d572c8545c2d97becde64515caba4',
}
ROLLOUT_TV_HEADER_SHA256 = 'bcfbcefdc62e4c720ed39a0d18d3360e683df1d19b905a8f21282b17dece5155'


def test_the_functions_are_exported_and_bound():
    _lib, L = lib_loaded()
    names = header_functions(HEADER)
    assert names == sorted(_lib.ROLLOUT_TV_EST_SYMBOLS) == FUNCTIONS
    older = (_lib.SYMBOLS + _lib.POLISH_SYMBOLS + _lib.MODEL_SYMBOLS + _lib.ADJOINT_SYMBOLS + _lib.ADJOINT_MODEL_SYMBOLS + _lib.ROLLOUT_SYMBOLS +
             _lib.ROLLOUT_EST_SYMBOLS + _lib.ADJOINT_BOUNDS_SYMBOLS + _lib.RICCATI_SYMBOLS + _lib.ROLLOUT_TV_SYMBOLS)
    assert not set(names) & set(older)
    assert _lib.ROLLOUT_TV_SYMBOLS == ['mpcqp_rollout_tv', 'mpcqp_rollout_tv_tape_bytes', 'mpcqp_rollout_adjoint_tv', 'mpcqp_rollout_tv_get_slot']      # (as it was)
    for n in names:
        assert hasattr(L, n) and getattr(L, n).argtypes is not None and getattr(L, n).restype is C.c_int, n
    assert _lib.has_rollout_tv_est(L)


def test_the_structs_mirror_the_header():
    from pympc_amd import _lib
    fields = ctypes_struct(_lib.EstTraj)
    assert fields == header_struct(HEADER, 'mpcqp_est_traj')
    assert [n for n, _ in fields] == ['struct_size', 'nentries', 'Lgain_traj']
    assert C.sizeof(_lib.EstTraj) == 8 + 8
    fields = ctypes_struct(_lib.RolloutTVEstIO)
    assert fields == header_struct(HEADER, 'mpcqp_rollout_tv_est_io')
    assert [n for n, _ in fields] == ['struct_size', 'reserved', 'd_Ae_entries', 'd_Be_entries', 'd_L_entries']
    assert C.sizeof(_lib.RolloutTVEstIO) == 8 + 3 * 8
    for taken in ('mpcqp_loop', 'mpcqp_model_traj', 'mpcqp_rollout_adjoint_io', 'mpcqp_rollout_est_io', 'mpcqp_adjoint_model_io', 'mpcqp_adjoint_bounds_io',
                  'mpcqp_rollout_tv_io'):
        assert taken in HEADER, taken                      # (the structs of the older headers the new calls take)


def test_include_and_include_ext_are_untouched():
    digests = dict(OLDER_HEADERS, **NEWER_HEADERS)
    digests.update({'mpcqp_adjoint.h': ADJOINT_HEADER_SHA256, 'mpcqp_adjoint_model.h': ADJOINT_MODEL_HEADER_SHA256})
    for name, digest in digests.items():
        assert hashlib.sha256(open(os.path.join(ROOT, 'include', name), 'rb').read()).hexdigest() == digest, name
    assert sorted(os.listdir(os.path.join(ROOT, 'include'))) == sorted(digests)
    assert os.listdir(os.path.join(ROOT, 'include_ext')) == ['mpcqp_rollout_tv.h']
    assert hashlib.sha256(open(os.path.join(ROOT, 'include_ext', 'mpcqp_rollout_tv.h'), 'rb').read()).hexdigest() == ROLLOUT_TV_HEADER_SHA256
    assert os.listdir(os.path.join(ROOT, 'include_ext2')) == ['mpcqp_rollout_tv_est.h']
    from pympc_amd import _lib
    assert C.sizeof(_lib.RolloutAdjointIO) == 4 + 4 + 8 * 8 and C.sizeof(_lib.AdjointModelIO) == 4 + 4 + 7 * 8      # the structs the new calls take, as they were
    assert C.sizeof(_lib.AdjointBoundsIO) == 8 + 6 * 8 and C.sizeof(_lib.ModelTraj) == 16 + 2 * 8
    assert C.sizeof(_lib.RolloutEstIO) == 8 + 8 * 8 and C.sizeof(_lib.RolloutTVIO) == 8 + 4 * 8


def test_the_calls_check_their_arguments_without_a_handle():
    _lib, L = lib_loaded()
    io, lo, eo, mo, bo = _lib.RolloutAdjointIO(), _lib.Loop(), _lib.RolloutEstIO(), _lib.AdjointModelIO(), _lib.AdjointBoundsIO()
    to, xo, mt, et = _lib.RolloutTVIO(), _lib.RolloutTVEstIO(), _lib.ModelTraj(), _lib.EstTraj()
    n = C.c_int64()
    for call in (L.mpcqp_mpc_loop_tv_est, L.mpcqp_rollout_tv_est):
        assert call(None, 3, C.byref(lo), C.byref(mt), C.byref(et)) == -1
        assert call(None, 3, None, None, None) == -1
    assert L.mpcqp_rollout_tv_est_tape_bytes(None, 3, 1, 2, C.byref(n)) == -1
    assert L.mpcqp_rollout_adjoint_tv_est(None, C.byref(io), C.byref(eo), C.byref(mo), C.byref(bo), C.byref(to), C.byref(xo)) == -1
    assert L.mpcqp_rollout_adjoint_tv_est(None, None, None, None, None, None, None) == -1
    assert L.mpcqp_rollout_tv_est_get_gain(None, 0, None) == -1


def test_the_combination_against_the_cpu_twin_is_refused(twin):
    from pympc_amd import _lib, fixtures, BatchMPCController
    from pympc_amd.kalman import BatchLinearStateEstimator
    assert not _lib.has_rollout_tv_est(twin)
    kw = fixtures.point_mass()
    Kb = BatchMPCController(**repeated(kw, 2, uminus1=None, eps_feas=kw.get('eps_feas', 1e6)))      # (u_{-1}: the constructor's default)
    Kb.setup()
    tr = Kb.run(2)                                         # everything else works as before
    assert tr['x'].shape == (3, 2, 2)
    nx, nu = Kb.nx, Kb.nu
    Cm, Lg = np.zeros((2, 1, nx)), np.zeros((2, nx, 1))
    est = BatchLinearStateEstimator(np.array(Kb.x0_rh, dtype=float).reshape(2, nx), Kb.Ad, Kb.Bd, Cm, Lg)
    count, Ad, xh, Lbefore = Kb.solve_count, Kb.Ad, est.x.copy(), est.L
    sched = (np.stack([Kb.Ad, Kb.Ad]), None, 1)
    Lt = np.zeros((2, 2, nx, 1))
    for call in (lambda: Kb.run(2, estimator=est, model_traj=sched), lambda: Kb.run(2, estimator=est, model_traj=sched, L_traj=Lt),
                 lambda: Kb.rollout_tv_est(2, sched, est, L_traj=Lt)):
        with pytest.raises(NotImplementedError, match='mpcqp_rollout_tv_est'):
            call()
        assert Kb.solve_count == count and Kb.Ad is Ad and np.array_equal(est.x, xh) and est.L is Lbefore      # a refused call has not moved anything on
    bp = Kb.prob
    ed = dict(C=Cm, L=Lg, x_true=est.x_true)
    for call in (lambda: bp.mpc_run_tv_est(2, sched, ed), lambda: bp.rollout_tv_est(2, sched, ed), lambda: bp.rollout_tv_est_tape_bytes(2, 1, 1),
                 lambda: bp.rollout_tv_est_gain(0)):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(ValueError):
        Kb.run(2, L_traj=Lt)                               # a gain schedule without estimator and model schedule
