"""include/mpcqp_adjoint.h -- adjoint derivatives beside the C ABI of include/mpcqp.h: exported by the HIP library, bound by pympc_amd._lib
outside SYMBOLS, its structs mirrored field by field, its defaults as documented, the three older headers untouched; a library without it
(the CPU twin) makes the Python methods raise NotImplementedError.  No GPU needed."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from util import repeated
from abi import ROOT, header, header_struct, header_functions, lib_loaded, OLDER_HEADERS, twin      # noqa: F401  (twin: a fixture)

ADJOINT_HEADER = header('mpcqp_adjoint.h')


def test_adjoint_functions_exported_and_bound():
    _lib, L = lib_loaded()
    names = header_functions(ADJOINT_HEADER)
    assert names == sorted(_lib.ADJOINT_SYMBOLS)
    assert not set(names) & set(_lib.SYMBOLS + _lib.POLISH_SYMBOLS + _lib.MODEL_SYMBOLS)      # the older lists are unchanged
    for n in names:
        assert hasattr(L, n), n
        assert getattr(L, n).argtypes is not None, n      # bound with a prototype
    assert _lib.has_adjoint(L)


def test_adjoint_structs_mirror_the_header():
    from pympc_amd import _lib
    kind = lambda t: 'double' if t is C.c_double else ('int32' if t in (C.c_int32, C.c_int) else 'ptr')
    assert [(n, kind(t)) for n, t in _lib.AdjointSettings._fields_] == header_struct(ADJOINT_HEADER, 'mpcqp_adjoint_settings')
    assert C.sizeof(_lib.AdjointSettings) == 4 + 4 + 8 + 8 + 4 + 4
    assert [(n, kind(t)) for n, t in _lib.AdjointIO._fields_] == header_struct(ADJOINT_HEADER, 'mpcqp_adjoint_io')
    assert C.sizeof(_lib.AdjointIO) == 4 + 4 + 9 * 8


def test_adjoint_defaults():
    _lib, L = lib_loaded()
    s = _lib.AdjointSettings()
    L.mpcqp_adjoint_default_settings(C.byref(s))
    assert s.struct_size == C.sizeof(_lib.AdjointSettings)
    assert (s.delta, s.refine_iter, s.weak_tol, s.extra_iter, s.reserved) == (1e-6, 3, 1e-6, 60, 0)


def test_the_older_headers_are_unchanged():
    for name, digest in OLDER_HEADERS.items():
        data = open(os.path.join(ROOT, 'include', name), 'rb').read()
        assert hashlib.sha256(data).hexdigest() == digest, name


def test_adjoint_calls_check_their_arguments_without_a_handle():
    _lib, L = lib_loaded()
    s = _lib.AdjointSettings()
    L.mpcqp_adjoint_default_settings(C.byref(s))
    io = _lib.AdjointIO()
    assert L.mpcqp_set_adjoint(None, C.byref(s)) == -1
    assert L.mpcqp_adjoint(None, C.byref(io)) == -1
    assert L.mpcqp_gains(None, None, None, None, None) == -1
    assert L.mpcqp_get_adjoint_info(None, None, None, None) == -1


def test_adjoint_settings_are_not_solver_or_polish_settings():
    from pympc_amd import solver
    for k in ('weak_tol', 'refine_iter'):
        assert k not in solver._SETTING_NAMES and k not in solver._POLISH_SETTINGS
        with pytest.raises(TypeError):
            solver.make_settings(**{k: 1})


def test_adjoint_against_the_cpu_twin_is_refused(twin):
    from pympc_amd import _lib, fixtures, MPCController, BatchMPCController
    assert not _lib.has_adjoint(twin)
    kw = fixtures.point_mass()
    K = MPCController(**kw)
    K.setup()
    assert K.res.info.status == 'solved'                 # everything else works as before
    with pytest.raises(NotImplementedError):
        K.gains()
    bp = K.prob.batch_problem
    for call in (lambda: bp.adjoint(g_u0=np.ones((1, bp.nu))), lambda: bp.gains(), lambda: bp.adjoint_info(), lambda: bp.set_adjoint(delta=1e-5)):
        with pytest.raises(NotImplementedError):
            call()
    Kb = BatchMPCController(**repeated(kw, 2, uminus1=None, eps_feas=kw.get('eps_feas', 1e6)))      # (u_{-1}: the constructor's default)
    Kb.setup()
    with pytest.raises(NotImplementedError):
        Kb.gains()
    with pytest.raises(NotImplementedError):
        Kb.adjoint(g_u0=np.ones((2, 1)))
