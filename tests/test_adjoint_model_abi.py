"""include/mpcqp_adjoint_model.h -- the model gradients beside include/mpcqp_adjoint.h: exported by the HIP library, bound by pympc_amd._lib
outside the older symbol lists, its struct mirrored field by field, mpcqp_adjoint_io and the older headers untouched; a library without
it (the CPU twin) makes the Python methods raise NotImplementedError.  No GPU needed."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from util import repeated
from abi import ROOT, header, header_struct, header_functions, lib_loaded, OLDER_HEADERS, ADJOINT_HEADER_SHA256, twin      # noqa: F401  (twin: a fixture)

HEADER = header('mpcqp_adjoint_model.h')


def test_the_function_is_exported_and_bound():
    _lib, L = lib_loaded()
    names = header_functions(HEADER)
    assert names == sorted(_lib.ADJOINT_MODEL_SYMBOLS) == ['mpcqp_adjoint_model']
    assert not set(names) & set(_lib.SYMBOLS + _lib.POLISH_SYMBOLS + _lib.MODEL_SYMBOLS + _lib.ADJOINT_SYMBOLS)
    assert hasattr(L, 'mpcqp_adjoint_model') and L.mpcqp_adjoint_model.argtypes is not None
    assert _lib.has_adjoint_model(L)


def test_the_struct_mirrors_the_header():
    from pympc_amd import _lib
    kind = lambda t: 'double' if t is C.c_double else ('int32' if t in (C.c_int32, C.c_int) else 'ptr')
    fields = [(n, kind(t)) for n, t in _lib.AdjointModelIO._fields_]
    assert fields == header_struct(HEADER, 'mpcqp_adjoint_model_io')
    assert [n for n, _ in fields] == ['struct_size', 'batch_sum'] + ['d_' + n for n in _lib.ADJOINT_MODEL_NAMES]
    assert C.sizeof(_lib.AdjointModelIO) == 4 + 4 + 7 * 8


def test_the_adjoint_header_and_the_older_ones_are_unchanged():
    data = open(os.path.join(ROOT, 'include', 'mpcqp_adjoint.h'), 'rb').read()
    assert hashlib.sha256(data).hexdigest() == ADJOINT_HEADER_SHA256
    for name, digest in OLDER_HEADERS.items():
        assert hashlib.sha256(open(os.path.join(ROOT, 'include', name), 'rb').read()).hexdigest() == digest, name
    from pympc_amd import _lib
    assert C.sizeof(_lib.AdjointIO) == 4 + 4 + 9 * 8           # mpcqp_adjoint_io as it was
    assert [n for n, _ in _lib.AdjointIO._fields_] == ['struct_size', 'reserved', 'g_w', 'g_u0', 'd_x0', 'd_uminus1', 'd_xref', 'd_uref', 'd_q', 'd_l', 'd_u']


def test_the_call_checks_its_arguments_without_a_handle():
    _lib, L = lib_loaded()
    io, mo = _lib.AdjointIO(), _lib.AdjointModelIO()
    assert L.mpcqp_adjoint_model(None, C.byref(io), C.byref(mo)) == -1
    assert L.mpcqp_adjoint_model(None, None, None) == -1


def test_model_gradients_against_the_cpu_twin_are_refused(twin):
    from pympc_amd import _lib, fixtures, MPCController, BatchMPCController
    assert not _lib.has_adjoint_model(twin)
    kw = fixtures.point_mass()
    K = MPCController(**kw)
    K.setup()
    assert K.res.info.status == 'solved'                 # everything else works as before
    with pytest.raises(NotImplementedError, match='mpcqp_adjoint'):
        K.adjoint(g_u0=np.ones(1), want=('Ad',))
    bp = K.prob.batch_problem
    with pytest.raises(NotImplementedError):
        bp.adjoint(g_u0=np.ones((1, bp.nu)), want=('Ad', 'Qx'), batch_sum=True)
    Kb = BatchMPCController(**repeated(kw, 2, uminus1=None, eps_feas=kw.get('eps_feas', 1e6)))      # (u_{-1}: the constructor's default)
    Kb.setup()
    with pytest.raises(NotImplementedError):
        Kb.adjoint(g_u0=np.ones((2, 1)), want=('Bd',))
