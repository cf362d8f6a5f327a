"""include/mpcqp_adjoint_model.h -- the model gradients beside include/mpcqp_adjoint.h: exported by the HIP library, bound by pympc_amd._lib
outside the older symbol lists, its struct mirrored field by field, mpcqp_adjoint_io and the older headers untouched; a library without
it (the CPU twin) makes the Python methods raise NotImplementedError.  No GPU needed."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

from test_abi_layout import _strip_comments
from test_adjoint_abi import _lib_loaded, twin, OLDER_HEADERS      # noqa: F401  (twin: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'mpcqp_adjoint_model.h')).read()
ADJOINT_HEADER_SHA256 = 'e0292e51830ab2f92d7424665564e3b43597b7adc9f9423074a940eb6387a585'


def _struct(name, text):
    """[(field, kind)] of `typedef struct { ... } name;` in ``text``, kind in {'double', 'int32', 'ptr'} (the parser of
    tests/test_abi_layout.py, on a header of its own)."""
    body = re.search(r'typedef struct \{([^{}]*)\}\s*%s\s*;' % name, _strip_comments(text)).group(1)
    fields = []
    for decl in body.split(';'):
        decl = ' '.join(decl.split())
        if not decl:
            continue
        m = re.match(r'(const )?(double|int32_t)\s*(.*)', decl)
        assert m, decl
        for item in m.group(3).split(','):
            item = item.strip()
            fields.append((item.lstrip('* ').strip(), 'ptr' if item.startswith('*') else ('double' if m.group(2) == 'double' else 'int32')))
    return fields


def test_the_function_is_exported_and_bound():
    _lib, L = _lib_loaded()
    text = re.sub(r'typedef struct \{.*?\}\s*\w+\s*;', '', _strip_comments(HEADER), flags=re.S)
    names = sorted(set(re.findall(r'\b(mpcqp_\w+)\s*\(', text)))
    assert names == sorted(_lib.ADJOINT_MODEL_SYMBOLS) == ['mpcqp_adjoint_model']
    assert not set(names) & set(_lib.SYMBOLS + _lib.POLISH_SYMBOLS + _lib.MODEL_SYMBOLS + _lib.ADJOINT_SYMBOLS)
    assert hasattr(L, 'mpcqp_adjoint_model') and L.mpcqp_adjoint_model.argtypes is not None
    assert _lib.has_adjoint_model(L)


def test_the_struct_mirrors_the_header():
    from pympc_amd import _lib
    kind = lambda t: 'double' if t is C.c_double else ('int32' if t in (C.c_int32, C.c_int) else 'ptr')
    fields = [(n, kind(t)) for n, t in _lib.AdjointModelIO._fields_]
    assert fields == _struct('mpcqp_adjoint_model_io', HEADER)
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
    _lib, L = _lib_loaded()
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
    st = lambda a: np.stack([np.asarray(a, dtype=float)] * 2)
    Kb = BatchMPCController(st(kw['Ad']), st(kw['Bd']), Np=kw['Np'], x0=st(kw['x0']), xref=st(kw['xref']), uref=st(kw['uref']),
                            Qx=st(kw['Qx']), QxN=st(kw['QxN']), Qu=st(kw['Qu']), QDu=st(kw['QDu']), xmin=st(kw['xmin']), xmax=st(kw['xmax']),
                            umin=st(kw['umin']), umax=st(kw['umax']), Dumin=st(kw['Dumin']), Dumax=st(kw['Dumax']), eps_feas=kw.get('eps_feas', 1e6))
    Kb.setup()
    with pytest.raises(NotImplementedError):
        Kb.adjoint(g_u0=np.ones((2, 1)), want=('Bd',))
