"""The polish specification (tests/polish_ref.py) against the certified optima, on the CPU and before any GPU is involved: the oracle
(OSQP restated in C, no scaling) solves every golden fixture at pyMPC's tolerance eps 1e-3, and polishing its iterate with identity
scaling must reproduce x* of opt_<name>.npz to 1e-8 relative on the fixtures whose active set the iterate gets right at that tolerance.

Measured here: OSQP's acceptance rule compares residuals only, so it also accepts a polished point whose active-set guess was wrong
(cart_pole: both residuals ~1e-16, multipliers of the wrong sign on a few inequality rows, x 1.5e-2 away from x*), and a right guess
reaches x* to ~2e-8 only on the badly scaled accel_brake fixtures and cart_pole_kalman.  EXACT lists the fixtures where polishing the
eps-1e-3 iterate gives x* to 1e-8, ACCEPTED those where it is accepted at all; tests/test_gpu_polish.py holds the device to both."""
import numpy as np
import pytest

from util import golden_names, load_golden
from polish_ref import golden_qp, polish, EXACT, ACCEPTED, EXACT_SCALED

EPS = 1e-3


def oracle_polish(name, eps=EPS):
    """(QP, oracle result, polish) of fixture `name`: the oracle's solve at `eps`, polished from its iterate with identity scaling."""
    from oracle.osqp_oracle import OSQP
    P, q, A, l, u = qp = golden_qp(load_golden(name))
    o = OSQP()
    o.setup(P, q, A, np.clip(l, -1e30, 1e30), np.clip(u, -1e30, 1e30), scaling=0, eps_abs=eps, eps_rel=eps, max_iter=100000)
    r = o.solve()
    x, z, y, _ = o.iterate_state()
    ones_n, ones_m = np.ones(P.shape[0]), np.ones(A.shape[0])
    pol = polish(P, q, A, l, u, x, z, y, ones_n, ones_m, 1.0, r.info.pri_res, r.info.dua_res)
    return qp, r, pol


@pytest.mark.parametrize('name', golden_names())
def test_polished_oracle_iterate_reaches_the_optimum(name):
    _, r, pol = oracle_polish(name)
    assert r.info.status == 'solved'
    opt = np.load('%s/golden/opt_%s.npz' % (__import__('os').path.dirname(__file__), name))
    xs = opt['x']
    err = np.abs(pol['x'] - xs).max() / max(1.0, np.abs(xs).max())
    assert (pol['status_polish'] == 1) == (name in ACCEPTED), (name, pol['status_polish'])
    assert (pol['status_polish'] == 1 and err <= 1e-8) == (name in EXACT), (name, err)
    if pol['status_polish'] == 1:
        assert pol['pri_res'] < r.info.pri_res or pol['dua_res'] < r.info.dua_res


@pytest.mark.parametrize('name', golden_names())
def test_polish_in_the_ruiz_scaling(name):
    """The oracle with OSQP's default scaling, polished in its own scaling (D, E, c): the run tests/test_gpu_polish.py mirrors."""
    from oracle.osqp_oracle import OSQP
    P, q, A, l, u = golden_qp(load_golden(name))
    o = OSQP()
    o.setup(P, q, A, np.clip(l, -1e30, 1e30), np.clip(u, -1e30, 1e30), eps_abs=EPS, eps_rel=EPS, max_iter=100000)
    r = o.solve()
    x, z, y, _ = o.iterate_state()
    D, E, c = o.scaling()
    pol = polish(P, q, A, l, u, x, z, y, D, E, c, r.info.pri_res, r.info.dua_res)
    xs = np.load('%s/golden/opt_%s.npz' % (__import__('os').path.dirname(__file__), name))['x']
    err = np.abs(pol['x'] - xs).max() / max(1.0, np.abs(xs).max())
    assert (pol['status_polish'] == 1) == (name in ACCEPTED), (name, pol['status_polish'])
    assert (pol['status_polish'] == 1 and err <= 1e-8) == (name in EXACT_SCALED), (name, err)


def test_unpolished_iterate_is_far_from_the_optimum():
    """What polishing is for: at eps 1e-3 the raw ADMM iterate of the headline shape is nowhere near 1e-8 of x*."""
    _, r, pol = oracle_polish('random_12_4_30')
    xs = np.load('%s/golden/opt_random_12_4_30.npz' % __import__('os').path.dirname(__file__))['x']
    assert np.abs(r.x - xs).max() > 1e-6 * max(1.0, np.abs(xs).max())
    assert pol['status_polish'] == 1 and np.abs(pol['x'] - xs).max() <= 1e-8 * max(1.0, np.abs(xs).max())


def test_rejection_rule_keeps_a_worse_point_out():
    """A huge regularization with no refinement leaves the polished point worse than the iterate: rejected."""
    from oracle.osqp_oracle import OSQP
    P, q, A, l, u = golden_qp(load_golden('random_12_4_30'))
    o = OSQP()
    o.setup(P, q, A, np.clip(l, -1e30, 1e30), np.clip(u, -1e30, 1e30), scaling=0, eps_abs=EPS, eps_rel=EPS, max_iter=100000)
    r = o.solve()
    x, z, y, _ = o.iterate_state()
    pol = polish(P, q, A, l, u, x, z, y, np.ones(P.shape[0]), np.ones(A.shape[0]), 1.0, r.info.pri_res, r.info.dua_res,
                 delta=10.0, refine_iter=0)
    assert pol['status_polish'] == -1
