"""include/mpcqp_adjoint.h -- adjoint derivatives beside the C ABI of include/mpcqp.h: exported by the HIP library, bound by pympc_amd._lib
outside SYMBOLS, its structs mirrored field by field, its defaults as documented, the three older headers untouched; a library without it
(the CPU twin) makes the Python methods raise NotImplementedError.  No GPU needed."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from test_abi_layout import header_struct, _strip_comments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADJOINT_HEADER = open(os.path.join(ROOT, 'include', 'mpcqp_adjoint.h')).read()

# the headers this extension sits beside, as they were before it (sha256 of the files)
OLDER_HEADERS = {
    'mpcqp.h': '9b65550ae4f89a6a8ef2d36876ae97a0bc26d31d994514d8c3a1c1ab8e0832a8',
    'mpcqp_polish.h': '8fdf6b5c286dbd74132ab41a8a18616ed4bb5d73233d1fd209293d46fbc682ad',
    'mpcqp_model.h': '2803bb5b65ee660e7da727e459a53997cd7f6d3d0f702b18a04a1bc6b7bb2692',
}


def _adjoint_functions():
    text = re.sub(r'typedef struct \{.*?\}\s*\w+\s*;', '', _strip_comments(ADJOINT_HEADER), flags=re.S)
    return sorted(set(re.findall(r'\b(mpcqp_\w+)\s*\(', text)))


def _lib_loaded():
    import __graft_entry__ as g
    from pympc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib, _lib.load()


def _struct(name):
    import test_abi_layout
    old = test_abi_layout.HEADER
    test_abi_layout.HEADER = ADJOINT_HEADER
    try:
        return header_struct(name)
    finally:
        test_abi_layout.HEADER = old


def test_adjoint_functions_exported_and_bound():
    _lib, L = _lib_loaded()
    names = _adjoint_functions()
    assert names == sorted(_lib.ADJOINT_SYMBOLS)
    assert not set(names) & set(_lib.SYMBOLS + _lib.POLISH_SYMBOLS + _lib.MODEL_SYMBOLS)      # the older lists are unchanged
    for n in names:
        assert hasattr(L, n), n
        assert getattr(L, n).argtypes is not None, n      # bound with a prototype
    assert _lib.has_adjoint(L)


def test_adjoint_structs_mirror_the_header():
    from pympc_amd import _lib
    kind = lambda t: 'double' if t is C.c_double else ('int32' if t in (C.c_int32, C.c_int) else 'ptr')
    assert [(n, kind(t)) for n, t in _lib.AdjointSettings._fields_] == _struct('mpcqp_adjoint_settings')
    assert C.sizeof(_lib.AdjointSettings) == 4 + 4 + 8 + 8 + 4 + 4
    assert [(n, kind(t)) for n, t in _lib.AdjointIO._fields_] == _struct('mpcqp_adjoint_io')
    assert C.sizeof(_lib.AdjointIO) == 4 + 4 + 9 * 8


def test_adjoint_defaults():
    _lib, L = _lib_loaded()
    s = _lib.AdjointSettings()
    L.mpcqp_adjoint_default_settings(C.byref(s))
    assert s.struct_size == C.sizeof(_lib.AdjointSettings)
    assert (s.delta, s.refine_iter, s.weak_tol, s.extra_iter, s.reserved) == (1e-6, 3, 1e-6, 60, 0)


def test_the_older_headers_are_unchanged():
    for name, digest in OLDER_HEADERS.items():
        data = open(os.path.join(ROOT, 'include', name), 'rb').read()
        assert hashlib.sha256(data).hexdigest() == digest, name


def test_adjoint_calls_check_their_arguments_without_a_handle():
    _lib, L = _lib_loaded()
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


@pytest.fixture
def twin():
    from pympc_amd import _lib
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'oracle'), 'libmpcqp_cpu.so'])
    old = (_lib.LIB_PATH, _lib._lib)
    _lib.LIB_PATH, _lib._lib = os.path.join(ROOT, 'oracle', 'libmpcqp_cpu.so'), None
    try:
        yield _lib.load()
    finally:
        _lib.LIB_PATH, _lib._lib = old


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
    st = lambda a: np.stack([np.asarray(a, dtype=float)] * 2)
    Kb = BatchMPCController(st(kw['Ad']), st(kw['Bd']), Np=kw['Np'], x0=st(kw['x0']), xref=st(kw['xref']), uref=st(kw['uref']),
                            Qx=st(kw['Qx']), QxN=st(kw['QxN']), Qu=st(kw['Qu']), QDu=st(kw['QDu']), xmin=st(kw['xmin']), xmax=st(kw['xmax']),
                            umin=st(kw['umin']), umax=st(kw['umax']), Dumin=st(kw['Dumin']), Dumax=st(kw['Dumax']), eps_feas=kw.get('eps_feas', 1e6))
    Kb.setup()
    with pytest.raises(NotImplementedError):
        Kb.gains()
    with pytest.raises(NotImplementedError):
        Kb.adjoint(g_u0=np.ones((2, 1)))
