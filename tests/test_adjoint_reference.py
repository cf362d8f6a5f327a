"""The mathematics of the adjoint derivatives (include/mpcqp_adjoint.h), pinned on the CPU before any GPU is involved: the numpy / scipy
restatement tests/adjoint_ref.py against central finite differences of the CPU oracle, against the closed-form unconstrained law, and the
active-set and weak-row rules on the golden fixtures.  tests/test_gpu_adjoint.py holds the device to the same restatement.

STRICT are the fixtures with strict complementarity at the optimum (no weakly active row): values are compared on these.  DEGENERATE are
the six with weakly active rows (a kink of the control law: no derivative exists): only 'reports n_weak > 0' is asserted on them.  The lists
are fixed by name; a fixture does not move between them to make a test pass."""

import numpy as np
import pytest

from polish_ref import active_set as polish_active_set
import adjoint_ref as ar
from adjoint_cases import STRICT, DEGENERATE, NO_INEQUALITY_ACTIVE, oracle_qp, solve_golden
import closed_form


def _dims(kw):
    nx, nu = np.asarray(kw['Bd']).shape
    return nx, nu, (kw['Np'] + 1) * nx


def _gains(name, eps=1e-11):
    kw, (P, q, A, l, u), r, (x, z, y), (D, E, c) = solve_golden(name, eps)
    nx, nu, ou = _dims(kw)
    return kw, ar.gains(P, A, l, u, x, z, y, D, E, c, ar.parameter_maps(kw, kw.attrs), ou, nu)


def test_the_fixture_lists_are_the_golden_set():
    from util import golden_names
    assert sorted(STRICT + DEGENERATE) == golden_names() and len(STRICT) == 15 and len(DEGENERATE) == 6


# ---- (a) the restatement against central finite differences of the oracle -----------------------------------------------------------------
@pytest.mark.parametrize('name', STRICT)
def test_restatement_against_finite_differences(name):
    """du0/dx0 against central differences, h = 1e-5 on l[:nx] = u[:nx] = -x0, of the oracle at eps 1e-11.  Tolerance 1e-4 max(1, |J|_inf):
    finite-difference noise is about 2 (solver error ~1e-10) / h ~ 1e-5, this is ten times that."""
    kw, (P, q, A, l, u), r, (x, z, y), (D, E, c) = solve_golden(name, 1e-11)
    nx, nu, ou = _dims(kw)
    K = ar.gains(P, A, l, u, x, z, y, D, E, c, ar.parameter_maps(kw, kw.attrs), ou, nu)
    assert K['n_weak'] == 0
    h = 1e-5
    J = np.zeros((nu, nx))
    for j in range(nx):
        us = []
        for s in (+1.0, -1.0):
            l2, u2 = np.clip(l, -1e30, 1e30), np.clip(u, -1e30, 1e30)
            l2[j] -= s * h; u2[j] -= s * h                    # x0[j] += s h
            rr = oracle_qp(P, q, A, l2, u2, 1e-11).solve()     # (a cold solve each, like the base point: both ends of a difference follow the
                                                               #  same iteration path, so their solver errors largely cancel; warm-started
                                                               #  from one another they do not -- 2.8e-3 on cart_pole_kalman)
            assert rr.info.status == 'solved'
            us.append(rr.x[ou:ou + nu].copy())
        J[:, j] = (us[0] - us[1]) / (2 * h)
    err = np.abs(K['K_x0'] - J).max()
    print('%s: |K_x0 - FD|_inf = %.3e, |J|_inf = %.3e' % (name, err, np.abs(J).max()))
    assert err <= 1e-4 * max(1.0, np.abs(J).max()), (name, err)


# ---- (b) no inequality active: the closed-form law ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NO_INEQUALITY_ACTIVE)
def test_restatement_equals_the_unconstrained_law(name):
    kw, K = _gains(name)
    nx, nu, _ = _dims(kw)
    assert K['n_active'] == (kw['Np'] + 1) * nx and K['n_weak'] == 0        # the dynamics rows alone
    base = dict(kw)
    base.setdefault('uminus1', np.array(kw['uref'], dtype=float))
    u_of = lambda over: closed_form.unconstrained_mpc(**dict(base, **over))[0][0]
    u0 = u_of({})
    for key, arg in (('K_x0', 'x0'), ('K_um1', 'uminus1'), ('K_xref', 'xref'), ('K_uref', 'uref')):
        v0 = np.array(base[arg], dtype=float)
        J = np.zeros((nu, v0.size))
        for j in range(v0.size):                               # the law is affine: a unit step gives the column exactly
            v = v0.copy().ravel(); v[j] += 1.0
            J[:, j] = u_of({arg: v.reshape(v0.shape)}) - u0
        err = np.abs(K[key] - J).max()
        assert err <= 1e-8 * max(1.0, np.abs(J).max()), (name, key, err)


# ---- (c) the active-set rule on the iterate -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', STRICT)
def test_active_set_rule_finds_the_true_set_at_parity_tolerance(name):
    kw, (P, q, A, l, u), r9, (x, z, y), (D, E, c) = solve_golden(name, 1e-9)
    _, _, r11, (x2, z2, y2), _ = solve_golden(name, 1e-11)
    eq = np.clip(l, -1e30, 1e30) == np.clip(u, -1e30, 1e30)
    pl, pu = polish_active_set(A, l, u, x, z, y, D, E, c)
    el, eu = ar.exact_active_rows(A, l, u, r11.x, r11.y)
    assert np.array_equal(pl | pu | eq, el | eu), name
    assert np.array_equal(pl & ~eq, el & ~eq) and np.array_equal(pu & ~eq, eu & ~eq), name
    low, upp = ar.active_rows(A, l, u, x, z, y, D, E, c)
    assert np.array_equal(low, el) and np.array_equal(upp, eu)
    assert ar.count_weak(l, u, z, y) == 0 and ar.count_weak(l, u, z2, y2) == 0


# ---- (d) the degenerate fixtures report their weak rows -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', DEGENERATE)
def test_degenerate_fixtures_report_weak_rows(name):
    kw, (P, q, A, l, u), r9, (x, z, y), _ = solve_golden(name, 1e-9)
    assert ar.count_weak(l, u, z, y) > 0, name


def test_restatement_conventions():
    """d_l / d_u: lower-active and equality rows in d_l, upper-active rows in d_u, inactive rows 0; dL/dq = -r_w; the chain for x0 is
    -r_y[:nx] (l[:nx] = u[:nx] = -x0, read off the builder)."""
    kw, (P, q, A, l, u), r, (x, z, y), (D, E, c) = solve_golden('point_mass', 1e-11)
    nx, nu, ou = _dims(kw)
    g = np.random.default_rng(0).standard_normal(P.shape[0])
    res = ar.adjoint(P, A, l, u, x, z, y, D, E, c, g, ar.parameter_maps(kw, kw.attrs))
    low, upp = res['low'], res['upp']
    assert upp.any() or (low & (l != u)).any()
    assert np.all(res['d_l'][~low] == 0) and np.all(res['d_u'][~upp] == 0)
    assert np.array_equal(res['d_q'], -res['r_w'])
    assert np.allclose(res['x0'], -res['r_y'][:nx], rtol=0, atol=1e-12)
    # the KKT system it claims to solve
    Pd, Ad = P.toarray(), A.toarray()
    act = low | upp
    assert np.abs(Pd @ res['r_w'] + Ad[act].T @ res['r_y'][act] - g).max() <= 1e-9 * max(1.0, np.abs(g).max())
    assert np.abs(Ad[act] @ res['r_w']).max() <= 1e-9
