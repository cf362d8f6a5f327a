"""MPCController.update_model on the host, with the CPU oracle (oracle/osqp_ref.c) as ``prob``: a solver without an update_model of its own,
so the controller takes the generic route -- a fresh ``type(prob)()`` set up with the rebuilt matrices and warm-started from res.x, res.y."""
import warnings

import numpy as np
import pytest

from util import load_golden, golden_kwargs, oracle_controller
from ltv_models import new_model, with_model, MODEL_FIELDS

NAMES = ['cart_pole', 'quadcopter_nc', 'random_12_4_30', 'random_20_8_12_hard', 'point_mass']


def _same_sparse(a, b):
    a, b = a.tocsc(), b.tocsc()
    return a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(a.data, b.data)


@pytest.mark.parametrize('name', NAMES)
def test_public_qp_is_that_of_a_controller_constructed_with_the_new_model(name):
    kw = golden_kwargs(load_golden(name))
    new = new_model(kw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K = oracle_controller(kw); K.setup()
        K.update_model(**new)
        Kn = oracle_controller(with_model(kw, new)); Kn.setup(solve=False)
    assert _same_sparse(K.P, Kn.P) and _same_sparse(K.A, Kn.A)
    assert np.array_equal(K.q, Kn.q) and np.array_equal(K.l, Kn.l) and np.array_equal(K.u, Kn.u)
    for k in MODEL_FIELDS:
        assert np.array_equal(getattr(K, k), new[k]), k


@pytest.mark.parametrize('name', NAMES)
def test_result_is_fresh_setup_warm_start_solve_written_by_hand(name):
    from oracle.osqp_oracle import OSQP
    kw = golden_kwargs(load_golden(name))
    new = new_model(kw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K = oracle_controller(kw); K.setup()
        x, y = K.res.x.copy(), K.res.y.copy()
        old_prob = K.prob
        K.update_model(**new)
        assert K.prob is not old_prob and isinstance(K.prob, OSQP)
        Kn = oracle_controller(with_model(kw, new)); Kn.setup(solve=False)
        O = OSQP()
        O.setup(Kn.P, Kn.q, Kn.A, Kn.l, Kn.u, warm_start=True, eps_abs=Kn.eps_rel, eps_rel=Kn.eps_abs)
        O.warm_start(x=x, y=y)
        r = O.solve()
    assert np.array_equal(K.res.x, r.x) and np.array_equal(K.res.y, r.y)
    assert (K.res.info.status, K.res.info.iter, K.res.info.rho_updates, K.res.info.obj_val) == (r.info.status, r.info.iter, r.info.rho_updates, r.info.obj_val)
    assert K.res.info.status == 'solved'


def test_update_model_in_the_middle_of_a_closed_loop_uses_the_current_step_data():
    """After update() and output() the controller's x0_rh / uminus1_rh have moved on: q, l, u are rebuilt for them."""
    kw = golden_kwargs(load_golden('cart_pole'))
    new = new_model(kw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K = oracle_controller(kw); K.setup()
        x = np.array(kw['x0'], dtype=float)
        for _ in range(3):
            u = K.output()
            x = kw['Ad'] @ x + kw['Bd'] @ u
            K.update(x, u)
        u = K.output()
        K.update_model(Ad=new['Ad'], Bd=new['Bd'], solve=False)
        Kn = oracle_controller(with_model(kw, dict(Ad=new['Ad'], Bd=new['Bd'], x0=x, uminus1=u))); Kn.setup(solve=False)
    assert _same_sparse(K.A, Kn.A) and _same_sparse(K.P, Kn.P)
    assert np.array_equal(K.q, Kn.q) and np.array_equal(K.l, Kn.l) and np.array_equal(K.u, Kn.u)


@pytest.mark.parametrize('fields', [('Bd',), ('xmax', 'umin', 'Dumax'), ('Qx', 'QDu'), ('uref',), ('eps_feas',)])
def test_partial_updates_leave_the_other_attributes_alone(fields):
    kw = golden_kwargs(load_golden('random_12_4_30'))
    new = dict(new_model(kw), uref=0.05 * np.ones(4), eps_feas=2e5)
    attrs = MODEL_FIELDS + ('uref', 'eps_feas', 'x0', 'xref', 'uminus1', 'Np', 'Nc', 'eps_rel', 'eps_abs')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K = oracle_controller(kw); K.setup()
        before = {k: getattr(K, k) for k in attrs}
        K.update_model(**{k: new[k] for k in fields})
    for k in attrs:
        if k in fields:
            assert np.array_equal(getattr(K, k), new[k]), k
        else:
            assert getattr(K, k) is before[k], k
    if 'uref' in fields:
        assert K.u_failure is K.uref
    if 'eps_feas' in fields:
        assert np.array_equal(K.Qeps.toarray(), 2e5 * np.eye(12))
    assert K.res.info.status == 'solved'


def test_invalid_shapes_raise_the_constructors_errors():
    from pympc_amd import MPCController
    from pympc_amd.controller import _ERR
    kw = golden_kwargs(load_golden('random_12_4_30'))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K = oracle_controller(kw); K.setup()
    nx, nu = 12, 4
    bad = dict(Ad=np.ones((nx, nx + 1)), Bd=np.ones((nx + 1, nu)), Qx=np.eye(nx + 1), QxN=np.ones((nx + 1, nx)), Qu=np.eye(nu + 1), QDu=np.ones((nu, nu + 1)),
               xmin=np.ones(nx + 1), xmax=np.ones((nx, 1)), umin=np.ones(nu - 1), umax=np.ones((2, 2)), Dumin=np.ones((nu, 1)), Dumax=np.ones(nu + 1),
               uref=np.ones(nu + 2))
    good = dict(Ad=np.eye(nx), Bd=np.ones((nx, nu)), Np=5, Qx=np.eye(nx))
    prob, P, res = K.prob, K.P, K.res
    for k, v in bad.items():
        with pytest.raises(ValueError) as e_upd:
            K.update_model(**{k: v})
        with pytest.raises(ValueError) as e_ctor:
            MPCController(**dict(good, **{k: v}))
        assert str(e_upd.value) == str(e_ctor.value), k
        if k in _ERR:
            assert str(e_upd.value) == _ERR[k]
        assert getattr(K, k) is kw[k] or np.array_equal(getattr(K, k), kw[k])      # a refused call changes nothing
    assert K.prob is prob and K.P is P and K.res is res
    with pytest.raises(ValueError):
        K.update_model()


def test_before_setup_only_the_attributes_change():
    from pympc_amd import MPCController
    kw = golden_kwargs(load_golden('point_mass'))
    K = MPCController(**kw)
    Bd2 = 2.0 * np.asarray(kw['Bd'])
    K.update_model(Bd=Bd2)
    assert K.Bd is Bd2 and K.prob is None and K.P is None and K.res is None
