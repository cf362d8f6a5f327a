"""include/mpcqp_adjoint_bounds.h -- the bound gradients beside the adjoint, model-gradient and rollout headers: exported by the HIP
library, bound by pympc_amd._lib outside the older symbol lists, its struct mirrored field by field, every older header untouched; a
library without it (the CPU twin) makes the Python methods raise NotImplementedError.  No GPU needed."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from util import repeated
from abi import (ROOT, header, header_struct, ctypes_struct, header_functions, lib_loaded, OLDER_HEADERS, ADJOINT_HEADER_SHA256,
                 ADJOINT_MODEL_HEADER_SHA256, twin)      # noqa: F401  (twin: a fixture)

HEADER = header('mpcqp_adjoint_bounds.h')
# the headers that came after tests/abi.py's, as this extension found them (sha256 of the files)
NEWER_HEADERS = {
    'mpcqp_rollout.h': 'b77eed88f091515afe45b3d05f1a4f24fd6a15d507578c3a0892371e6e55f978',
    'mpcqp_rollout_est.h': 'bdceeaa9c89cb16b1c95a9fbe8f60c04d1a7fb72cbf675f9b3529beaca3f142d',
    'mpcqp_riccati.h': '9a711292b530a9700c4c96e5520ae7ed296b77044e82876778c817f79e9fe6a2',
}


def test_the_functions_are_exported_and_bound():
    _lib, L = lib_loaded()
    names = header_functions(HEADER)
    assert names == sorted(_lib.ADJOINT_BOUNDS_SYMBOLS) == ['mpcqp_adjoint_bounds', 'mpcqp_rollout_adjoint_bounds']
    older = (_lib.SYMBOLS + _lib.POLISH_SYMBOLS + _lib.MODEL_SYMBOLS + _lib.ADJOINT_SYMBOLS + _lib.ADJOINT_MODEL_SYMBOLS + _lib.ROLLOUT_SYMBOLS +
             _lib.ROLLOUT_EST_SYMBOLS + _lib.RICCATI_SYMBOLS)
    assert not set(names) & set(older)
    for n in names:
        assert hasattr(L, n) and getattr(L, n).argtypes is not None and getattr(L, n).restype is C.c_int, n
    assert _lib.has_adjoint_bounds(L)
    assert _lib.ADJOINT_BOUNDS_NAMES == ('xmin', 'xmax', 'umin', 'umax', 'Dumin', 'Dumax')


def test_the_struct_mirrors_the_header():
    from pympc_amd import _lib
    fields = ctypes_struct(_lib.AdjointBoundsIO)
    assert fields == header_struct(HEADER, 'mpcqp_adjoint_bounds_io')
    assert [n for n, _ in fields] == ['struct_size', 'batch_sum'] + ['d_' + n for n in _lib.ADJOINT_BOUNDS_NAMES]
    assert C.sizeof(_lib.AdjointBoundsIO) == 8 + 6 * 8 == 56


def test_every_older_header_is_unchanged():
    digests = dict(OLDER_HEADERS, **NEWER_HEADERS)
    digests.update({'mpcqp_adjoint.h': ADJOINT_HEADER_SHA256, 'mpcqp_adjoint_model.h': ADJOINT_MODEL_HEADER_SHA256})
    for name, digest in digests.items():
        assert hashlib.sha256(open(os.path.join(ROOT, 'include', name), 'rb').read()).hexdigest() == digest, name
    assert sorted(os.listdir(os.path.join(ROOT, 'include'))) == sorted(list(digests) + ['mpcqp_adjoint_bounds.h'])
    from pympc_amd import _lib
    assert C.sizeof(_lib.AdjointIO) == 4 + 4 + 9 * 8 and C.sizeof(_lib.AdjointModelIO) == 4 + 4 + 7 * 8      # the structs the new calls take, as they were
    assert C.sizeof(_lib.RolloutAdjointIO) == 4 + 4 + 8 * 8 and C.sizeof(_lib.RolloutEstIO) == 8 + 8 * 8


def test_the_calls_check_their_arguments_without_a_handle():
    _lib, L = lib_loaded()
    io, mo, bo = _lib.AdjointIO(), _lib.AdjointModelIO(), _lib.AdjointBoundsIO()
    assert L.mpcqp_adjoint_bounds(None, C.byref(io), C.byref(mo), C.byref(bo)) == -1
    assert L.mpcqp_adjoint_bounds(None, None, None, None) == -1
    ro, eo = _lib.RolloutAdjointIO(), _lib.RolloutEstIO()
    assert L.mpcqp_rollout_adjoint_bounds(None, C.byref(ro), C.byref(eo), C.byref(mo), C.byref(bo)) == -1
    assert L.mpcqp_rollout_adjoint_bounds(None, None, None, None, None) == -1


def test_bound_gradients_against_the_cpu_twin_are_refused(twin):
    from pympc_amd import _lib, fixtures, MPCController, BatchMPCController
    assert not _lib.has_adjoint_bounds(twin)
    kw = fixtures.point_mass()
    K = MPCController(**kw)
    K.setup()
    assert K.res.info.status == 'solved'                 # everything else works as before
    with pytest.raises(NotImplementedError, match='mpcqp_adjoint'):
        K.adjoint(g_u0=np.ones(1), want=('umax',))
    bp = K.prob.batch_problem
    for name in _lib.ADJOINT_BOUNDS_NAMES:
        with pytest.raises(NotImplementedError):
            bp.adjoint(g_u0=np.ones((1, bp.nu)), want=('x0', name), batch_sum=True)
    Kb = BatchMPCController(**repeated(kw, 2, uminus1=None, eps_feas=kw.get('eps_feas', 1e6)))      # (u_{-1}: the constructor's default)
    Kb.setup()
    with pytest.raises(NotImplementedError):
        Kb.adjoint(g_u0=np.ones((2, 1)), want=('Dumax',))
    assert Kb.status() == ['solved', 'solved']
