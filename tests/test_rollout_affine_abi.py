"""include_ext5/mpcqp_rollout_affine.h -- the taped rollout with an affine term in the prediction model and its reverse sweep -- in a directory of
its own beside include/ and include_ext/ .. include_ext4/: exported by the HIP library, bound by pympc_amd._lib in a symbol list of its own, its
struct mirrored field by field, the older directories and symbol groups untouched; a library without it (the CPU twin) makes every new Python
entry raise NotImplementedError.  (Argument errors through the C ABI need a handle, and a handle a device: tests/test_gpu_rollout_affine.py.)
No GPU needed."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from util import repeated
from abi import ROOT, header_struct, ctypes_struct, header_functions, lib_loaded, twin      # noqa: F401  (twin: a fixture)

HEADER = open(os.path.join(ROOT, 'include_ext5', 'mpcqp_rollout_affine.h')).read()
FUNCTIONS = ['mpcqp_gains_affine', 'mpcqp_rollout_adjoint_affine', 'mpcqp_rollout_affine', 'mpcqp_rollout_affine_get_slot', 'mpcqp_rollout_affine_get_tape', 'mpcqp_rollout_affine_tape_bytes']
# the four extension directories as this one found them (sha256 of the files; include/ itself is pinned file by file in tests/test_rollout_tv_abi.py)
OLDER = {('include_ext', 'mpcqp_rollout_tv.h'): 'bcfbcefdc62e4c720ed39a0d18d3360e683df1d19b905a8f21282b17dece5155',
         ('include_ext2', 'mpcqp_rollout_tv_est.h'): '8c53da53581a3c71a859098fd6e49d23be87600db153b9bd1be7effceb1d8055',
         ('include_ext3', 'mpcqp_riccati_traj.h'): '8ce462fb1358a3776e3f584b16394bdd1d4d9aa4ddf1be7b69ab37375e474af6',
         ('include_ext4', 'mpcqp_affine.h'): '1d9f8da43e8739f8081d453c2a999829f6dbab797b0fca1e6c012314447dd398'}


def test_the_functions_are_exported_and_bound():
    _lib, L = lib_loaded()
    names = header_functions(HEADER)
    assert names == sorted(_lib.ROLLOUT_AFFINE_SYMBOLS) == FUNCTIONS
    older = (_lib.SYMBOLS + _lib.POLISH_SYMBOLS + _lib.MODEL_SYMBOLS + _lib.ADJOINT_SYMBOLS + _lib.ADJOINT_MODEL_SYMBOLS + _lib.ROLLOUT_SYMBOLS + _lib.ROLLOUT_EST_SYMBOLS +
             _lib.ADJOINT_BOUNDS_SYMBOLS + _lib.RICCATI_SYMBOLS + _lib.ROLLOUT_TV_SYMBOLS + _lib.ROLLOUT_TV_EST_SYMBOLS + _lib.RICCATI_TRAJ_SYMBOLS + _lib.AFFINE_SYMBOLS)
    assert not set(names) & set(older)
    assert sorted(_lib.AFFINE_SYMBOLS) == ['mpcqp_adjoint_affine', 'mpcqp_get_affine', 'mpcqp_mpc_loop_affine', 'mpcqp_set_affine']      # (the group before this one, as it was)
    assert len(_lib.ROLLOUT_TV_SYMBOLS) == 4 and len(_lib.ROLLOUT_SYMBOLS) == 6 and len(_lib.ADJOINT_SYMBOLS) == 5
    for n in names:
        assert hasattr(L, n) and getattr(L, n).argtypes is not None and getattr(L, n).restype is C.c_int, n
    assert len(L.mpcqp_rollout_affine.argtypes) == 5 and len(L.mpcqp_rollout_adjoint_affine.argtypes) == 6
    assert len(L.mpcqp_rollout_affine_tape_bytes.argtypes) == 6 and len(L.mpcqp_rollout_affine_get_slot.argtypes) == 3
    assert len(L.mpcqp_gains.argtypes) == 5 and len(L.mpcqp_gains_affine.argtypes) == 6      # (mpcqp_gains itself is untouched)
    assert _lib.has_rollout_affine(L)


def test_the_struct_mirrors_the_header():
    from pympc_amd import _lib
    fields = ctypes_struct(_lib.RolloutAffineIO)
    assert fields == header_struct(HEADER, 'mpcqp_rollout_affine_io')
    assert [n for n, _ in fields] == ['struct_size', 'reserved', 'd_d_slots']
    assert C.sizeof(_lib.RolloutAffineIO) == 8 + 8
    for taken in ('mpcqp_loop', 'mpcqp_model_traj', 'mpcqp_affine_traj', 'mpcqp_rollout_adjoint_io', 'mpcqp_adjoint_model_io', 'mpcqp_adjoint_bounds_io', 'mpcqp_rollout_tv_io'):
        assert taken in HEADER, taken                      # (the structs of the older headers the new calls take)
    assert 'without the offset' in HEADER and 'tau(k)' in HEADER


def test_the_older_header_directories_are_untouched():
    headers = lambda d: sorted(f for f in os.listdir(os.path.join(ROOT, d)) if f.endswith('.h'))      # (a stray backup file beside a header is no change of the ABI)
    for (d, name), digest in OLDER.items():
        assert headers(d) == [name]
        assert hashlib.sha256(open(os.path.join(ROOT, d, name), 'rb').read()).hexdigest() == digest, name
    assert headers('include_ext5') == ['mpcqp_rollout_affine.h']
    from pympc_amd import _lib
    assert C.sizeof(_lib.RolloutAdjointIO) == 8 + 8 * 8 and C.sizeof(_lib.RolloutTVIO) == 8 + 4 * 8 and C.sizeof(_lib.AffineTraj) == 16 + 8      # as they were


def test_the_calls_check_their_arguments_without_a_handle():
    _lib, L = lib_loaded()
    lo, at, io, ao = _lib.Loop(), _lib.AffineTraj(), _lib.RolloutAdjointIO(), _lib.RolloutAffineIO()
    d, n = np.zeros(4), C.c_int64(7)
    p = C.c_void_p(d.ctypes.data)
    assert L.mpcqp_rollout_affine(None, 3, C.byref(lo), None, C.byref(at)) == -1
    assert L.mpcqp_rollout_affine(None, 3, C.byref(lo), None, None) == -1
    assert L.mpcqp_rollout_affine_tape_bytes(None, 3, 0, 1, 1, C.byref(n)) == -1 and n.value == 7
    assert L.mpcqp_rollout_adjoint_affine(None, C.byref(io), None, None, None, C.byref(ao)) == -1
    assert L.mpcqp_rollout_affine_get_slot(None, 0, p) == -1 and L.mpcqp_rollout_affine_get_tape(None, 0, p) == -1
    assert L.mpcqp_gains_affine(None, p, None, None, None, p) == -1
    assert not d.any()


def test_the_sweep_has_no_instantiation_of_its_own():
    """The affine sweep is a runtime path of k_rollout_adjoint / k_rollout_adjoint_tv: the build has the four sweeps at the four stage widths it had."""
    import re
    from util import kernel_resources
    lib_loaded()
    sweeps = sorted(k for k in kernel_resources() if re.match(r'_Z\d+k_rollout_adjoint', k))
    assert len(sweeps) == 16, sweeps
    assert not [k for k in kernel_resources() if 'affine' in k and 'rollout' in k]


def test_every_new_python_entry_against_the_cpu_twin_is_refused(twin):
    from pympc_amd import _lib, fixtures, BatchMPCController
    assert not _lib.has_rollout_affine(twin)
    kw = fixtures.point_mass()
    Kb = BatchMPCController(**repeated(kw, 2, uminus1=None, eps_feas=kw.get('eps_feas', 1e6)))
    Kb.setup()
    tr = Kb.run(2)                                         # everything else works as before
    assert tr['x'].shape == (3, 2, 2)
    count = Kb.solve_count
    dt = np.zeros((2, 2, 2))
    calls = (lambda: Kb.rollout_affine(2, d_traj=dt), lambda: Kb.rollout_affine(2), lambda: Kb.prob.rollout_affine(2, d_traj=dt, d_hold=2),
             lambda: Kb.prob.rollout_affine_slot(0), lambda: Kb.prob.rollout_affine_tape_bytes(2, 1, d_hold=1),
             lambda: Kb.rollout_adjoint(g_u=np.ones((2, 2, 1)), want=('d0',)), lambda: Kb.prob.rollout_adjoint(g_u=np.ones((2, 2, 1)), want=('lam', 'd_traj')))
    for call in calls:
        with pytest.raises(NotImplementedError, match='mpcqp_rollout_affine'):
            call()
    assert Kb.solve_count == count
    if _lib.has_adjoint(twin):                             # (gains() asks for K_d only of a library that has the call, and only with a term)
        assert 'K_d' not in Kb.gains()
