"""include/mpcqp_rollout.h -- the taped rollout and its reverse sweep beside the older headers: exported by the HIP library, bound by
pympc_amd._lib in a symbol list of its own, its struct mirrored field by field, every older header untouched; a library without it (the
CPU twin) makes the Python methods raise NotImplementedError.  No GPU needed."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from util import repeated
from abi import ROOT, header, header_struct, header_functions, lib_loaded, OLDER_HEADERS, ADJOINT_HEADER_SHA256, ADJOINT_MODEL_HEADER_SHA256
from abi import twin      # noqa: F401  (a fixture)

HEADER = header('mpcqp_rollout.h')
FUNCTIONS = ['mpcqp_get_rollout_info', 'mpcqp_rollout', 'mpcqp_rollout_adjoint', 'mpcqp_rollout_get_tape', 'mpcqp_rollout_release',
             'mpcqp_rollout_tape_bytes']


def test_the_functions_are_exported_and_bound():
    _lib, L = lib_loaded()
    names = header_functions(HEADER)
    assert names == sorted(_lib.ROLLOUT_SYMBOLS) == FUNCTIONS
    assert not set(names) & set(_lib.SYMBOLS + _lib.POLISH_SYMBOLS + _lib.MODEL_SYMBOLS + _lib.ADJOINT_SYMBOLS + _lib.ADJOINT_MODEL_SYMBOLS)
    for n in names:
        assert hasattr(L, n), n
        assert getattr(L, n).argtypes is not None and getattr(L, n).restype is C.c_int, n
    assert _lib.has_rollout(L)


def test_the_struct_mirrors_the_header():
    from pympc_amd import _lib
    kind = lambda t: 'double' if t is C.c_double else ('int32' if t in (C.c_int32, C.c_int) else 'ptr')
    fields = [(n, kind(t)) for n, t in _lib.RolloutAdjointIO._fields_]
    assert fields == header_struct(HEADER, 'mpcqp_rollout_adjoint_io')
    assert [n for n, _ in fields] == ['struct_size', 'no_reuse', 'G_x', 'G_u', 'lam', 'd_uminus1', 'd_uref', 'd_xref', 'd_Ap', 'd_Bp']
    assert C.sizeof(_lib.RolloutAdjointIO) == 4 + 4 + 8 * 8
    assert 'mpcqp_loop' in HEADER and 'mpcqp_adjoint_model_io' in HEADER      # (the forward call takes the loop's struct, the sweep the model gradients')


def test_every_older_header_is_unchanged():
    digest = lambda name: hashlib.sha256(open(os.path.join(ROOT, 'include', name), 'rb').read()).hexdigest()
    assert digest('mpcqp_adjoint.h') == ADJOINT_HEADER_SHA256
    assert digest('mpcqp_adjoint_model.h') == ADJOINT_MODEL_HEADER_SHA256
    for name, want in OLDER_HEADERS.items():
        assert digest(name) == want, name
    from pympc_amd import _lib
    assert C.sizeof(_lib.AdjointModelIO) == 4 + 4 + 7 * 8 and C.sizeof(_lib.AdjointIO) == 4 + 4 + 9 * 8


def test_the_calls_check_their_arguments_without_a_handle():
    _lib, L = lib_loaded()
    io, lo, mo = _lib.RolloutAdjointIO(), _lib.Loop(), _lib.AdjointModelIO()
    n = C.c_int64()
    assert L.mpcqp_rollout(None, 3, C.byref(lo)) == -1
    assert L.mpcqp_rollout_tape_bytes(None, 3, C.byref(n)) == -1
    assert L.mpcqp_rollout_release(None) == -1
    assert L.mpcqp_rollout_adjoint(None, C.byref(io), C.byref(mo)) == -1
    assert L.mpcqp_get_rollout_info(None, None, None, None, None) == -1
    assert L.mpcqp_rollout_get_tape(None, 0, None, None, None, None, None) == -1


def test_a_rollout_against_the_cpu_twin_is_refused(twin):
    from pympc_amd import _lib, fixtures, BatchMPCController
    assert not _lib.has_rollout(twin)
    kw = fixtures.point_mass()
    Kb = BatchMPCController(**repeated(kw, 2, uminus1=None, eps_feas=kw.get('eps_feas', 1e6)))      # (u_{-1}: the constructor's default)
    Kb.setup()
    tr = Kb.run(2)                                         # everything else works as before
    assert tr['x'].shape == (3, 2, 2)
    count = Kb.solve_count
    with pytest.raises(NotImplementedError, match='mpcqp_rollout'):
        Kb.rollout(2)
    assert Kb.solve_count == count                          # a refused rollout has not moved the controller on
    with pytest.raises(NotImplementedError):
        Kb.rollout_adjoint(g_u=np.ones((2, 2, 1)))
    bp = Kb.prob
    for call in (lambda: bp.rollout(2), lambda: bp.rollout_adjoint(g_u=np.ones((2, 2, 1))), lambda: bp.rollout_info(), lambda: bp.rollout_tape(0),
                 lambda: bp.rollout_tape_bytes(2), lambda: bp.rollout_release()):
        with pytest.raises(NotImplementedError):
            call()
