"""include/mpcqp_model.h (mpcqp_update_model, mpcqp_mpc_loop_tv) is an extension BESIDE include/mpcqp.h: its prototypes are bound by
_lib.MODEL_SYMBOLS -- never by _lib.SYMBOLS, which stays the list of mpcqp.h --, its struct is mirrored field by field by _lib.ModelTraj,
and a library without it (the CPU twin under oracle/) still loads and runs the package, which then takes the generic route."""
import ctypes as C
import warnings

import numpy as np
import pytest

from util import load_golden, golden_kwargs
from abi import header, header_struct, header_functions, twin      # noqa: F401  (twin: a fixture)


def test_model_symbols_are_the_header_and_stay_out_of_the_core_list():
    from pympc_amd import _lib
    assert sorted(_lib.MODEL_SYMBOLS) == header_functions(header('mpcqp_model.h'))
    assert not set(_lib.MODEL_SYMBOLS) & set(_lib.SYMBOLS)
    assert not set(_lib.MODEL_SYMBOLS) & set(header_functions(header('mpcqp.h')))


def test_model_traj_mirrors_the_header():
    from pympc_amd import _lib
    kind = lambda t: 'double' if t is C.c_double else ('int32' if t in (C.c_int32, C.c_int) else 'ptr')
    assert [(n, kind(t)) for n, t in _lib.ModelTraj._fields_] == header_struct(header('mpcqp_model.h'), 'mpcqp_model_traj')
    assert C.sizeof(_lib.ModelTraj) == 4 * 4 + 2 * 8
    assert _lib.ModelTraj.Ad.offset == 16 and _lib.ModelTraj.Bd.offset == 24


def test_twin_lacks_the_model_symbols_and_the_package_still_loads(twin):
    from pympc_amd import _lib
    from pympc_amd.solver import BatchProblem
    assert all(hasattr(twin, s) for s in _lib.SYMBOLS)
    assert not any(hasattr(twin, s) for s in _lib.MODEL_SYMBOLS)
    assert not _lib.has_model_update() and not _lib.has_model_update(twin)
    bp = BatchProblem(1, 2, 1, 5)
    with pytest.raises(NotImplementedError):
        bp.update_model(Ad=np.eye(2)[None])
    with pytest.raises(NotImplementedError):
        bp.mpc_run(2, model_traj=(np.zeros((2, 1, 2, 2)), None, 1))


def test_controller_on_the_twin_takes_the_generic_route(twin):
    """A DeviceProblem whose library has no mpcqp_update_model: MPCController.update_model sets a fresh one up with the new matrices and
    warm-starts it from res.x, res.y -- the result is that of the same three calls written out by hand."""
    from pympc_amd import MPCController
    kw = golden_kwargs(load_golden('point_mass'))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K = MPCController(**kw); K.setup()
        old_prob, x, y = K.prob, K.res.x.copy(), K.res.y.copy()
        assert not K.prob.supports_update_model
        Bd2 = 1.1 * np.asarray(kw['Bd'])
        K.update_model(Bd=Bd2, umax=np.array([1.0]))
        assert K.prob is not old_prob and type(K.prob) is type(old_prob)
        K2 = MPCController(**dict(kw, Bd=Bd2, umax=np.array([1.0]))); K2.setup(solve=False)
        K2.prob.warm_start(x=x, y=y)
        K2.solve()
    assert np.array_equal(K.res.x, K2.res.x) and np.array_equal(K.res.y, K2.res.y)
    assert (K.res.info.status, K.res.info.iter) == (K2.res.info.status, K2.res.info.iter)
    assert K.res.info.status == 'solved'
