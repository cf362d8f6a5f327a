"""include/mpcqp_riccati.h -- the batched Riccati solver and its adjoint beside the older headers: exported by the HIP library, bound by
pympc_amd._lib in a symbol list of its own, its settings struct mirrored field by field, every older header untouched; a library without
it (the CPU twin) makes pympc_amd.riccati raise NotImplementedError.  No GPU needed."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from abi import ROOT, header, header_struct, ctypes_struct, header_functions, lib_loaded, OLDER_HEADERS, ADJOINT_HEADER_SHA256, ADJOINT_MODEL_HEADER_SHA256
from abi import twin      # noqa: F401  (a fixture)
from util import kernel_resources

HEADER = header('mpcqp_riccati.h')
FUNCTIONS = ['mpcqp_dare', 'mpcqp_dare_adjoint', 'mpcqp_riccati_default_settings']


def test_the_functions_are_exported_and_bound():
    _lib, L = lib_loaded()
    names = header_functions(HEADER)
    assert names == sorted(_lib.RICCATI_SYMBOLS) == FUNCTIONS
    older = (_lib.SYMBOLS + _lib.POLISH_SYMBOLS + _lib.MODEL_SYMBOLS + _lib.ADJOINT_SYMBOLS + _lib.ADJOINT_MODEL_SYMBOLS + _lib.ROLLOUT_SYMBOLS
             + _lib.ROLLOUT_EST_SYMBOLS)
    assert not set(names) & set(older)
    for n in names:
        assert hasattr(L, n), n
        assert getattr(L, n).argtypes is not None, n
    assert L.mpcqp_dare.restype is C.c_int and L.mpcqp_dare_adjoint.restype is C.c_int
    assert len(L.mpcqp_dare.argtypes) == 15 and len(L.mpcqp_dare_adjoint.argtypes) == 20
    assert _lib.has_riccati(L)


def test_the_struct_mirrors_the_header_and_its_defaults():
    _lib, L = lib_loaded()
    fields = ctypes_struct(_lib.RiccatiSettings)
    assert fields == header_struct(HEADER, 'mpcqp_riccati_settings')
    assert [n for n, _ in fields] == ['struct_size', 'max_iter', 'gain_form', 'reserved', 'tol']
    assert C.sizeof(_lib.RiccatiSettings) == 4 * 4 + 8
    s = _lib.RiccatiSettings()
    L.mpcqp_riccati_default_settings(C.byref(s))
    assert (s.struct_size, s.max_iter, s.gain_form, s.reserved, s.tol) == (24, 50, 0, 0, 1e-15)


def test_every_older_header_is_unchanged():
    digest = lambda name: hashlib.sha256(open(os.path.join(ROOT, 'include', name), 'rb').read()).hexdigest()
    assert digest('mpcqp_adjoint.h') == ADJOINT_HEADER_SHA256
    assert digest('mpcqp_adjoint_model.h') == ADJOINT_MODEL_HEADER_SHA256
    for name, want in OLDER_HEADERS.items():
        assert digest(name) == want, name


def test_the_calls_check_sizes_and_pointers_before_they_look_for_a_device():
    _lib, L = lib_loaded()
    ARG, UNSUPPORTED = -1, -4
    z = np.zeros(33 * 33)
    p = C.c_void_p(z.ctypes.data)
    st = np.zeros(1, dtype=np.int32)
    ps = C.c_void_p(st.ctypes.data)
    dare = lambda n, m, s=None, batch=1, A=p: L.mpcqp_dare(0, None, batch, n, m, s, A, p, p, p, p, p, ps, ps, p)
    adj = lambda n, m, G=p, d=p: L.mpcqp_dare_adjoint(0, None, 1, n, m, None, p, p, p, p, p, p, ps, G, G, d, d, d, d, ps)
    for call in (dare, adj):
        assert call(33, 1) == UNSUPPORTED and b'32' in L.mpcqp_last_error()
        assert call(1, 33) == UNSUPPORTED
        assert call(0, 1) == ARG and call(2, 0) == ARG
    assert dare(2, 1, batch=0) == ARG
    assert dare(2, 1, A=None) == ARG and b'must be given' in L.mpcqp_last_error()
    assert adj(2, 1, G=None) == ARG and b'seed' in L.mpcqp_last_error()
    assert adj(2, 1, d=None) == ARG
    s = _lib.RiccatiSettings()
    L.mpcqp_riccati_default_settings(C.byref(s))
    s.struct_size = 16
    assert dare(2, 1, C.byref(s)) == ARG and b'struct_size' in L.mpcqp_last_error()
    L.mpcqp_riccati_default_settings(C.byref(s))
    for field, value in (('max_iter', 0), ('gain_form', 2), ('tol', -1.0), ('tol', float('nan'))):
        L.mpcqp_riccati_default_settings(C.byref(s))
        setattr(s, field, value)
        assert dare(2, 1, C.byref(s)) == ARG, field


def test_the_build_has_the_four_kernels():
    """k_dare<NB> and k_dare_adjoint<NB>, NB = 16 and 32, in the resource remarks of the build, without scratch."""
    lib_loaded()
    ks = kernel_resources()
    for name in ('_Z6k_dareILi16EE', '_Z6k_dareILi32EE', '_Z14k_dare_adjointILi16EE', '_Z14k_dare_adjointILi32EE'):
        hit = [v for k, v in ks.items() if k.startswith(name)]
        assert len(hit) == 1, name
        assert int(hit[0]['ScratchSize']) == 0 and int(hit[0]['Occupancy']) >= 1, (name, hit[0])


def test_the_cpu_twin_has_no_riccati_solver(twin):
    from pympc_amd import _lib, riccati
    assert not _lib.has_riccati(twin)
    assert not any(hasattr(twin, s) for s in _lib.RICCATI_SYMBOLS)
    I2, b = np.eye(2), np.ones((2, 1))
    for call in (lambda: riccati.dare(I2, b, I2, np.eye(1)), lambda: riccati.dare_adjoint(I2, b, I2, np.eye(1), I2, b.T, G_X=I2),
                 lambda: riccati.kalman_gain(I2, b.T, I2, np.eye(1)), lambda: riccati.lqr_terminal(I2, b, I2, np.eye(1))):
        with pytest.raises(NotImplementedError, match='mpcqp_dare'):
            call()
