"""include_ext4/mpcqp_affine.h -- the affine term of the prediction model, x+ = Ad x + Bd u + d -- in a directory of its own beside include/,
include_ext/, include_ext2/ and include_ext3/: exported by the HIP library, bound by pympc_amd._lib in a symbol list of its own, its struct
mirrored field by field, the older directories untouched; a library without it (the CPU twin) makes every new Python entry raise
NotImplementedError.  (Argument errors through the C ABI need a handle, and a handle a device: tests/test_gpu_affine.py.)  No GPU needed."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from util import repeated
from abi import ROOT, header_struct, ctypes_struct, header_functions, lib_loaded, twin      # noqa: F401  (twin: a fixture)

HEADER = open(os.path.join(ROOT, 'include_ext4', 'mpcqp_affine.h')).read()
FUNCTIONS = ['mpcqp_adjoint_affine', 'mpcqp_get_affine', 'mpcqp_mpc_loop_affine', 'mpcqp_set_affine']
# the three extension directories as this one found them (sha256 of the files; include/ itself is pinned file by file in tests/test_rollout_tv_abi.py)
OLDER = {('include_ext', 'mpcqp_rollout_tv.h'): 'bcfbcefdc62e4c720ed39a0d18d3360e683df1d19b905a8f21282b17dece5155',
         ('include_ext2', 'mpcqp_rollout_tv_est.h'): '8c53da53581a3c71a859098fd6e49d23be87600db153b9bd1be7effceb1d8055',
         ('include_ext3', 'mpcqp_riccati_traj.h'): '8ce462fb1358a3776e3f584b16394bdd1d4d9aa4ddf1be7b69ab37375e474af6'}
INCLUDE = ['mpcqp.h', 'mpcqp_adjoint.h', 'mpcqp_adjoint_bounds.h', 'mpcqp_adjoint_model.h', 'mpcqp_model.h', 'mpcqp_polish.h', 'mpcqp_riccati.h',
           'mpcqp_rollout.h', 'mpcqp_rollout_est.h']


def test_the_functions_are_exported_and_bound():
    _lib, L = lib_loaded()
    names = header_functions(HEADER)
    assert names == sorted(_lib.AFFINE_SYMBOLS) == FUNCTIONS
    older = (_lib.SYMBOLS + _lib.POLISH_SYMBOLS + _lib.MODEL_SYMBOLS + _lib.ADJOINT_SYMBOLS + _lib.ADJOINT_MODEL_SYMBOLS + _lib.ROLLOUT_SYMBOLS + _lib.ROLLOUT_EST_SYMBOLS +
             _lib.ADJOINT_BOUNDS_SYMBOLS + _lib.RICCATI_SYMBOLS + _lib.ROLLOUT_TV_SYMBOLS + _lib.ROLLOUT_TV_EST_SYMBOLS + _lib.RICCATI_TRAJ_SYMBOLS)
    assert not set(names) & set(older)
    for n in names:
        assert hasattr(L, n) and getattr(L, n).argtypes is not None and getattr(L, n).restype is C.c_int, n
    assert len(L.mpcqp_set_affine.argtypes) == 3 and len(L.mpcqp_get_affine.argtypes) == 3
    assert len(L.mpcqp_mpc_loop_affine.argtypes) == 5 and len(L.mpcqp_adjoint_affine.argtypes) == 3
    assert _lib.has_affine(L)


def test_the_struct_mirrors_the_header():
    from pympc_amd import _lib
    fields = ctypes_struct(_lib.AffineTraj)
    assert fields == header_struct(HEADER, 'mpcqp_affine_traj')
    assert [n for n, _ in fields] == ['struct_size', 'hold', 'nentries', 'rows', 'd']
    assert C.sizeof(_lib.AffineTraj) == 16 + 8
    for taken in ('mpcqp_loop', 'mpcqp_model_traj', 'mpcqp_adjoint_io'):
        assert taken in HEADER, taken                      # (the structs of the older headers the new calls take)
    assert 'WITHOUT the' in HEADER and 'io->w' in HEADER   # (the loop's plant does not get the offset: said where the call is declared)


def test_the_older_header_directories_are_untouched():
    for (d, name), digest in OLDER.items():
        assert os.listdir(os.path.join(ROOT, d)) == [name]
        assert hashlib.sha256(open(os.path.join(ROOT, d, name), 'rb').read()).hexdigest() == digest, name
    assert sorted(os.listdir(os.path.join(ROOT, 'include'))) == INCLUDE
    assert os.listdir(os.path.join(ROOT, 'include_ext4')) == ['mpcqp_affine.h']
    from pympc_amd import _lib
    assert C.sizeof(_lib.AdjointIO) == 8 + 9 * 8 and C.sizeof(_lib.ModelTraj) == 16 + 2 * 8      # the structs the new calls take, as they were


def test_the_calls_check_their_arguments_without_a_handle():
    _lib, L = lib_loaded()
    lo, at, io = _lib.Loop(), _lib.AffineTraj(), _lib.AdjointIO()
    d, rows = np.zeros(4), C.c_int(7)
    p = C.c_void_p(d.ctypes.data)
    assert L.mpcqp_set_affine(None, p, 1) == -1
    assert L.mpcqp_get_affine(None, p, C.byref(rows)) == -1 and rows.value == 7
    assert L.mpcqp_mpc_loop_affine(None, 3, C.byref(lo), None, C.byref(at)) == -1
    assert L.mpcqp_mpc_loop_affine(None, 3, C.byref(lo), None, None) == -1      # (at == NULL: mpcqp_mpc_loop_tv, mt == NULL: mpcqp_mpc_loop)
    assert L.mpcqp_adjoint_affine(None, C.byref(io), p) == -1
    assert not d.any()


def test_the_kernel_of_the_gradient_is_in_the_build():
    from util import kernel_resources
    lib_loaded()
    hit = [v for k, v in kernel_resources().items() if k.startswith('_Z13k_affine_grad')]
    assert len(hit) == 1 and int(hit[0]['ScratchSize']) == 0, hit


def test_every_new_python_entry_against_the_cpu_twin_is_refused(twin):
    from pympc_amd import _lib, fixtures, BatchMPCController, MPCController
    from pympc_amd.solver import DeviceProblem
    assert not _lib.has_affine(twin)
    kw = fixtures.point_mass()
    Kb = BatchMPCController(**repeated(kw, 2, uminus1=None, eps_feas=kw.get('eps_feas', 1e6)))
    Kb.setup()
    tr = Kb.run(2)                                         # everything else works as before
    assert tr['x'].shape == (3, 2, 2)
    count = Kb.solve_count
    d, dt = np.zeros((2, 2)), np.zeros((2, 2, 2))
    calls = (lambda: Kb.set_affine(d), lambda: Kb.set_affine(None), lambda: Kb.affine(), lambda: Kb.update(Kb.x0, d=d), lambda: Kb.step(Kb.x0, d=d),
             lambda: Kb.adjoint(g_u0=np.ones((2, 1)), want=('d',)), lambda: Kb.prob.set_affine(d), lambda: Kb.prob.affine(), lambda: Kb.prob.affine_rows(),
             lambda: Kb.prob.mpc_run(2, d_traj=dt), lambda: Kb.prob.adjoint(g_u0=np.ones((2, 1)), want=('d',)))
    for call in calls:
        with pytest.raises(NotImplementedError, match='mpcqp_affine'):
            call()
    solves = Kb.solve_count
    with pytest.raises(NotImplementedError, match='mpcqp_affine'):
        Kb.run(2, d_traj=dt)
    assert count == solves                                 # (the refused update / step have not solved)
    K = MPCController(**kw)
    K.prob = DeviceProblem()
    K.setup()
    for call in (lambda: K.set_affine(np.zeros(2)), lambda: K.update(kw['x0'], d=np.zeros(2)), lambda: K.adjoint(g_u0=np.ones(1), want=('d',))):
        with pytest.raises(NotImplementedError, match='mpcqp_affine'):
            call()


def test_sharding_refuses_a_term():
    torch = pytest.importorskip('torch')
    from pympc_amd import sharding
    with pytest.raises(NotImplementedError, match='mpcqp_affine'):
        sharding.scatter_instances({'x0': torch.zeros(2, 3), 'd': torch.zeros(2, 3)}, {'x0': (3,), 'd': (3,)}, per_rank=2)
    out = sharding.scatter_instances({'x0': torch.ones(2, 3)}, {'x0': (3,)}, per_rank=2)      # (without one: as before)
    assert out['x0'].shape == (2, 3)
