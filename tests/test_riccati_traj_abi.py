"""include_ext3/mpcqp_riccati_traj.h -- the Riccati difference equation and its adjoint, in a directory of its own beside include/,
include_ext/ and include_ext2/: exported by the HIP library, bound by pympc_amd._lib in a symbol list of its own, the older directories
untouched, the arguments checked before the calls look for a device, the four kernels in the build's resource remarks.  No GPU needed."""
import ctypes as C
import hashlib
import os

import numpy as np

from abi import ROOT, header_functions, lib_loaded
from util import kernel_resources

HEADER = open(os.path.join(ROOT, 'include_ext3', 'mpcqp_riccati_traj.h')).read()
FUNCTIONS = ['mpcqp_dre', 'mpcqp_dre_adjoint']
ROLLOUT_TV_EST_HEADER_SHA256 = '8c53da53581a3c71a859098fd6e49d23be87600db153b9bd1be7effceb1d8055'
RICCATI_HEADER_SHA256 = '9a711292b530a9700c4c96e5520ae7ed296b77044e82876778c817f79e9fe6a2'


def test_the_functions_are_exported_and_bound():
    _lib, L = lib_loaded()
    names = header_functions(HEADER)
    assert names == sorted(_lib.RICCATI_TRAJ_SYMBOLS) == FUNCTIONS
    older = (_lib.SYMBOLS + _lib.POLISH_SYMBOLS + _lib.MODEL_SYMBOLS + _lib.ADJOINT_SYMBOLS + _lib.ADJOINT_MODEL_SYMBOLS + _lib.ROLLOUT_SYMBOLS + _lib.ROLLOUT_EST_SYMBOLS +
             _lib.ADJOINT_BOUNDS_SYMBOLS + _lib.RICCATI_SYMBOLS + _lib.ROLLOUT_TV_SYMBOLS + _lib.ROLLOUT_TV_EST_SYMBOLS)
    assert not set(names) & set(older)
    assert _lib.RICCATI_SYMBOLS == ['mpcqp_riccati_default_settings', 'mpcqp_dare', 'mpcqp_dare_adjoint']      # (as it was)
    for n in names:
        assert hasattr(L, n) and getattr(L, n).argtypes is not None and getattr(L, n).restype is C.c_int, n
    assert len(L.mpcqp_dre.argtypes) == 18 and len(L.mpcqp_dre_adjoint.argtypes) == 23
    assert _lib.has_riccati_traj(L)
    assert 'mpcqp_riccati_settings' in HEADER              # (the settings struct of include/mpcqp_riccati.h is the one the calls take)


def test_the_older_header_directories_are_untouched():
    digest = lambda *path: hashlib.sha256(open(os.path.join(ROOT, *path), 'rb').read()).hexdigest()
    assert os.listdir(os.path.join(ROOT, 'include_ext2')) == ['mpcqp_rollout_tv_est.h'] and os.listdir(os.path.join(ROOT, 'include_ext3')) == ['mpcqp_riccati_traj.h']
    assert digest('include_ext2', 'mpcqp_rollout_tv_est.h') == ROLLOUT_TV_EST_HEADER_SHA256
    assert digest('include', 'mpcqp_riccati.h') == RICCATI_HEADER_SHA256


def test_the_calls_check_sizes_and_pointers_before_they_look_for_a_device():
    _lib, L = lib_loaded()
    ARG, UNSUPPORTED = -1, -4
    z, st = np.zeros(8 * 33 * 33), np.zeros(1, dtype=np.int32)
    p, ps = C.c_void_p(z.ctypes.data), C.c_void_p(st.ctypes.data)

    def dre(n=2, m=1, T=7, A_steps=7, B_steps=1, X0=p, s=None, batch=1):
        return L.mpcqp_dre(0, None, batch, n, m, T, s, p, A_steps, p, B_steps, p, p, X0, p, p, ps, ps)

    def adj(n=2, m=1, T=7, A_steps=7, B_steps=1, G=p, d=p, batch=1):
        return L.mpcqp_dre_adjoint(0, None, batch, n, m, T, None, p, A_steps, p, B_steps, None, p, None, p, None, G, G, d, d, d, d, d)
    for call in (dre, adj):
        assert call(n=33) == UNSUPPORTED and b'32' in L.mpcqp_last_error()
        assert call(m=33) == UNSUPPORTED
        assert call(n=0) == ARG and call(m=0) == ARG and call(batch=0) == ARG and call(T=0, A_steps=0) == ARG
        assert call(A_steps=2) == ARG and b'A_steps' in L.mpcqp_last_error()
        assert call(B_steps=6) == ARG
    assert dre(X0=None) == ARG and b'must be given' in L.mpcqp_last_error()
    assert adj(G=None) == ARG and b'seed' in L.mpcqp_last_error()
    assert adj(d=None) == ARG and b'no gradient' in L.mpcqp_last_error()
    s = _lib.RiccatiSettings()
    L.mpcqp_riccati_default_settings(C.byref(s))
    s.struct_size = 16
    assert dre(s=C.byref(s)) == ARG and b'struct_size' in L.mpcqp_last_error()
    L.mpcqp_riccati_default_settings(C.byref(s))
    s.gain_form = 2
    assert dre(s=C.byref(s)) == ARG and b'gain_form' in L.mpcqp_last_error()
    assert not z.any() and not st.any()


def test_the_build_has_the_four_kernels_and_they_fit():
    """k_dre<NB> and k_dre_adjoint<NB>, NB = 16 and 32, in the resource remarks of the build, without scratch; the largest LDS block (19 blocks of
    32 x 32 doubles and the reductions' four) is within the 160 KB of a workgroup, as the header's static_assert says."""
    lib_loaded()
    ks = kernel_resources()
    for name in ('_Z5k_dreILi16EE', '_Z5k_dreILi32EE', '_Z13k_dre_adjointILi16EE', '_Z13k_dre_adjointILi32EE'):
        hit = [v for k, v in ks.items() if k.startswith(name)]
        assert len(hit) == 1, name
        assert int(hit[0]['ScratchSize']) == 0 and int(hit[0]['Occupancy']) >= 1, (name, hit[0])
    assert 8 * (19 * 32 * 32 + 4) <= 160 * 1024
    src = open(os.path.join(ROOT, 'pympc_amd', 'csrc', 'mpcqp_riccati_traj.h')).read()
    assert 'static_assert(ric_dre_lds<32>() <= 160 * 1024 && ric_dre_adjoint_lds<32>() <= 160 * 1024' in src and '19 * NB * NB + 4' in src
