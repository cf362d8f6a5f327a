"""include/mpcqp_polish.h -- OSQP's solution polishing beside the C ABI of include/mpcqp.h: exported by the HIP library, bound by
pympc_amd._lib outside SYMBOLS, its settings struct mirrored field by field, its defaults OSQP's; a library without it (the CPU twin)
refuses polish=True instead of ignoring it.  No GPU needed."""
import ctypes as C

import pytest

from abi import header, header_struct, header_functions, lib_loaded, twin      # noqa: F401  (twin: a fixture)

POLISH_HEADER = header('mpcqp_polish.h')


def test_polish_functions_exported_and_bound():
    _lib, L = lib_loaded()
    names = header_functions(POLISH_HEADER)
    assert names == sorted(_lib.POLISH_SYMBOLS)
    assert not set(names) & set(_lib.SYMBOLS)            # mpcqp.h's list is unchanged
    for n in names:
        assert hasattr(L, n), n
        assert getattr(L, n).argtypes is not None, n      # bound with a prototype
    assert _lib.has_polish(L)


def test_polish_struct_mirrors_the_header():
    from pympc_amd import _lib
    fields = header_struct(POLISH_HEADER, 'mpcqp_polish_settings')
    kind = lambda t: 'double' if t is C.c_double else ('int32' if t in (C.c_int32, C.c_int) else 'ptr')
    assert [(n, kind(t)) for n, t in _lib.PolishSettings._fields_] == fields
    assert C.sizeof(_lib.PolishSettings) == 4 + 4 + 8 + 4 + 4


def test_polish_defaults_are_osqps():
    _lib, L = lib_loaded()
    s = _lib.PolishSettings()
    L.mpcqp_polish_default_settings(C.byref(s))
    assert s.struct_size == C.sizeof(_lib.PolishSettings)
    assert (s.polish, s.delta, s.polish_refine_iter, s.reserved) == (0, 1e-6, 3, 0)


def test_polish_settings_are_no_longer_ignored():
    from pympc_amd import solver
    for k in ('polish', 'delta', 'polish_refine_iter'):
        assert k not in solver._IGNORED_SETTINGS
    with pytest.raises(TypeError):                        # not an mpcqp_settings field: the polish settings go their own way
        solver.make_settings(polish=True)


def test_set_polish_checks_its_arguments_without_a_handle():
    _lib, L = lib_loaded()
    s = _lib.PolishSettings()
    L.mpcqp_polish_default_settings(C.byref(s))
    assert L.mpcqp_set_polish(None, C.byref(s)) == -1
    assert L.mpcqp_polish(None) == -1
    assert L.mpcqp_get_polish_info(None, None) == -1


def test_polish_true_against_the_cpu_twin_is_refused(twin):
    from pympc_amd import _lib, fixtures, MPCController
    from pympc_amd.solver import BatchProblem
    assert not _lib.has_polish(twin)
    kw = fixtures.point_mass()
    with pytest.raises(NotImplementedError):
        BatchProblem(1, 2, 1, 10, polish=True)
    K = MPCController(**kw)
    K.solver_settings = dict(polish=True)
    with pytest.raises(NotImplementedError):
        K.setup()
    # polish off (or not mentioned) works as before, and reports status_polish 0
    K = MPCController(**kw)
    K.solver_settings = dict(polish=False, delta=1e-6)
    K.setup()
    assert K.res.info.status == 'solved' and K.res.info.status_polish == 0
