"""include_ext/mpcqp_rollout_tv.h -- the taped rollout under a model schedule and its reverse sweep, in a directory beside include/:
exported by the HIP library, bound by pympc_amd._lib in a symbol list of its own, its struct mirrored field by field, include/ untouched;
a library without it (the CPU twin) makes the Python methods raise NotImplementedError.  No GPU needed."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from util import repeated
from abi import (ROOT, header_struct, ctypes_struct, header_functions, lib_loaded, OLDER_HEADERS, ADJOINT_HEADER_SHA256,
                 ADJOINT_MODEL_HEADER_SHA256, twin)      # noqa: F401  (twin: a fixture)

HEADER = open(os.path.join(ROOT, 'include_ext', 'mpcqp_rollout_tv.h')).read()
FUNCTIONS = ['mpcqp_rollout_adjoint_tv', 'mpcqp_rollout_tv', 'mpcqp_rollout_tv_get_slot', 'mpcqp_rollout_tv_tape_bytes']
# include/ as this extension found it (sha256 of the files that came after tests/abi.py's)
NEWER_HEADERS = {
    'mpcqp_rollout.h': 'b77eed88f091515afe45b3d05f1a4f24fd6a15d507578c3a0892371e6e55f978',
    'mpcqp_rollout_est.h': 'bdceeaa9c89cb16b1c95a9fbe8f60c04d1a7fb72cbf675f9b3529beaca3f142d',
    'mpcqp_riccati.h': '9a711292b530a9700c4c96e5520ae7ed296b77044e82876778c817f79e9fe6a2',
    'mpcqp_adjoint_bounds.h': 'e059764945990e3cc234a8f3a959b8cda17d572c8545c2d97becde64515caba4',
}


def test_the_functions_are_exported_and_bound():
    _lib, L = lib_loaded()
    names = header_functions(HEADER)
    assert names == sorted(_lib.ROLLOUT_TV_SYMBOLS) == FUNCTIONS
    older = (_lib.SYMBOLS + _lib.POLISH_SYMBOLS + _lib.MODEL_SYMBOLS + _lib.ADJOINT_SYMBOLS + _lib.ADJOINT_MODEL_SYMBOLS + _lib.ROLLOUT_SYMBOLS +
             _lib.ROLLOUT_EST_SYMBOLS + _lib.ADJOINT_BOUNDS_SYMBOLS + _lib.RICCATI_SYMBOLS)
    assert not set(names) & set(older)
    for n in names:
        assert hasattr(L, n) and getattr(L, n).argtypes is not None and getattr(L, n).restype is C.c_int, n
    assert _lib.has_rollout_tv(L)


def test_the_struct_mirrors_the_header():
    from pympc_amd import _lib
    fields = ctypes_struct(_lib.RolloutTVIO)
    assert fields == header_struct(HEADER, 'mpcqp_rollout_tv_io')
    assert [n for n, _ in fields] == ['struct_size', 'reserved', 'd_Ad_slots', 'd_Bd_slots', 'd_Ap_entries', 'd_Bp_entries']
    assert C.sizeof(_lib.RolloutTVIO) == 8 + 4 * 8
    for taken in ('mpcqp_loop', 'mpcqp_model_traj', 'mpcqp_rollout_adjoint_io', 'mpcqp_adjoint_model_io', 'mpcqp_adjoint_bounds_io'):
        assert taken in HEADER, taken                      # (the structs of the older headers the new calls take)


def test_include_is_untouched():
    digests = dict(OLDER_HEADERS, **NEWER_HEADERS)
    digests.update({'mpcqp_adjoint.h': ADJOINT_HEADER_SHA256, 'mpcqp_adjoint_model.h': ADJOINT_MODEL_HEADER_SHA256})
    for name, digest in digests.items():
        assert hashlib.sha256(open(os.path.join(ROOT, 'include', name), 'rb').read()).hexdigest() == digest, name
    assert sorted(os.listdir(os.path.join(ROOT, 'include'))) == sorted(digests)
    assert os.listdir(os.path.join(ROOT, 'include_ext')) == ['mpcqp_rollout_tv.h']
    from pympc_amd import _lib
    assert C.sizeof(_lib.RolloutAdjointIO) == 4 + 4 + 8 * 8 and C.sizeof(_lib.AdjointModelIO) == 4 + 4 + 7 * 8      # the structs the new calls take, as they were
    assert C.sizeof(_lib.AdjointBoundsIO) == 8 + 6 * 8 and C.sizeof(_lib.ModelTraj) == 16 + 2 * 8


def test_the_calls_check_their_arguments_without_a_handle():
    _lib, L = lib_loaded()
    io, lo, mo, bo, to, mt = _lib.RolloutAdjointIO(), _lib.Loop(), _lib.AdjointModelIO(), _lib.AdjointBoundsIO(), _lib.RolloutTVIO(), _lib.ModelTraj()
    n = C.c_int64()
    assert L.mpcqp_rollout_tv(None, 3, C.byref(lo), C.byref(mt)) == -1
    assert L.mpcqp_rollout_tv(None, 3, None, None) == -1
    assert L.mpcqp_rollout_tv_tape_bytes(None, 3, 1, C.byref(n)) == -1
    assert L.mpcqp_rollout_adjoint_tv(None, C.byref(io), C.byref(mo), C.byref(bo), C.byref(to)) == -1
    assert L.mpcqp_rollout_adjoint_tv(None, None, None, None, None) == -1
    assert L.mpcqp_rollout_tv_get_slot(None, 0, None, None, None, None) == -1


def test_a_scheduled_rollout_against_the_cpu_twin_is_refused(twin):
    from pympc_amd import _lib, fixtures, BatchMPCController
    assert not _lib.has_rollout_tv(twin)
    kw = fixtures.point_mass()
    Kb = BatchMPCController(**repeated(kw, 2, uminus1=None, eps_feas=kw.get('eps_feas', 1e6)))      # (u_{-1}: the constructor's default)
    Kb.setup()
    tr = Kb.run(2)                                         # everything else works as before
    assert tr['x'].shape == (3, 2, 2)
    count, Ad = Kb.solve_count, Kb.Ad
    sched = (np.stack([Kb.Ad, Kb.Ad]), None, 1)
    with pytest.raises(NotImplementedError, match='mpcqp_rollout_tv'):
        Kb.rollout_tv(2, sched)
    assert Kb.solve_count == count and Kb.Ad is Ad          # a refused rollout has not moved the controller on
    bp = Kb.prob
    for call in (lambda: bp.rollout_tv(2, sched), lambda: bp.rollout_tv_tape_bytes(2, 1), lambda: bp.rollout_tv_slot(0)):
        with pytest.raises(NotImplementedError):
            call()
