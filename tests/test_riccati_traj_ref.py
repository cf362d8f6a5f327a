"""tests/riccati_traj_ref.py -- the CPU reference of the Riccati difference equation (include_ext3/mpcqp_riccati_traj.h) -- pinned: its two
forms against each other (what the device's bounds are made of: riccati_traj_ref.E_REF_TRAJ, E_REF_TRAJ_ADJ, the recorded figures, which
this test holds the reference to), its limit against scipy's algebraic solution, the scalar case by hand, its autograd gradients against
central differences, and the two conventions the designs rest on: the gain index of ``kalman_gain_traj`` against a textbook Kalman filter
through the loop's estimator, and ``lqr_traj``'s cost-to-go against a simulated closed loop.  The Python calls' refusals on the CPU twin.
No GPU needed.  Run with -s for the figures."""
import numpy as np
import pytest

import riccati_ref as rr
import riccati_traj_ref as tr
from abi import twin      # noqa: F401  (a fixture)

# the two forms differ by rounding alone, which moves with the BLAS build: the reference is held to ten times its recorded distance (a tenth
# of the factor the device gets), and to 1e-13 where the record is smaller than that
SLACK, FLOOR = 10.0, 1e-13
SEEDINGS = (('X', 0), ('K', 0), ('K', 1), ('XK', 0), ('XK', 1))      # (which outputs carry a seed, the gain form)


@pytest.mark.parametrize('name', tr.CASES)
def test_the_two_forms_agree(name):
    worst = 0.0
    for T in tr.STEPS:
        for pattern in tr.PATTERNS:
            m = tr.make(name, T, pattern)
            one, two = tr.run(m, T, 1), tr.run(m, T, 2)
            assert np.array_equal(one[0], np.swapaxes(one[0], -1, -2))
            worst = max([worst] + [tr.rel(a, b) for a, b in zip(one, two)])
    print('%-24s e_ref_traj %.1e' % (name, worst))
    assert worst <= max(SLACK * tr.E_REF_TRAJ[name], FLOOR), (worst, tr.E_REF_TRAJ[name])


@pytest.mark.parametrize('name', tr.CASES)
def test_autograd_through_the_two_forms_agrees(name):
    worst = 0.0
    for T in tr.STEPS:
        for pattern in tr.PATTERNS:
            m = tr.make(name, T, pattern)
            G_X, G_K = tr.seeds(name, T, *m['B'].shape[-2:])
            for which, gf in SEEDINGS:
                seed = (G_X if 'X' in which else None, G_K if 'K' in which else None, gf)
                one, two = tr.gradients(m, T, *seed, form=1), tr.gradients(m, T, *seed, form=2)
                for k in one:
                    if np.any(two[k]):
                        worst = max(worst, tr.rel(one[k], two[k]))
                    else:
                        assert not np.any(one[k]), k           # (a gain seed at T = 1 does not see Q)
                for k in ('Q', 'R', 'X0'):
                    assert np.array_equal(one[k], np.swapaxes(one[k], -1, -2))
    print('%-24s e_ref_traj_adj %.1e' % (name, worst))
    assert worst <= max(SLACK * tr.E_REF_TRAJ_ADJ[name], FLOOR), (worst, tr.E_REF_TRAJ_ADJ[name])


@pytest.mark.parametrize('name', tr.CASES)
def test_constant_matrices_reach_the_algebraic_solution(name):
    """With constant A, B the recursion converges to scipy.linalg.solve_discrete_are where the closed loop contracts; the number of steps is
    found here, on the reference, and every case of the list gets there well within the cap."""
    CAP = 400
    A, B, Q, R = rr.case(name)
    m = dict(A=A[None], B=B[None], Q=Q[None], R=R[None], X0=tr.initial(name, A.shape[0])[None])
    X, K, F = tr.run(m, CAP)
    Xs, Ks = rr.scipy_dare(A, B, Q, R, 0)
    Fs = rr.scipy_dare(A, B, Q, R, 1)[1]
    ok = lambda t: (rr.rel(X[t, 0], Xs) <= rr.bound(name, 0) and rr.rel(K[t - 1, 0], Ks) <= rr.bound(name, 1) and rr.rel(F[t - 1, 0], Fs) <= rr.bound(name, 2))
    T = next((t for t in range(1, CAP + 1) if ok(t)), None)
    print('%-24s reaches scipy\'s solution after %s steps' % (name, T))
    assert T is not None and ok(CAP)
    assert max(abs(np.linalg.eigvals(A - B @ Ks))) < 1.0


def test_scalar_against_the_hand_recursion():
    a, b, q, r = (M[0, 0] for M in rr.SCALAR)
    x = x0 = 0.37
    m = dict(A=[[[a]]], B=[[[b]]], Q=[[[q]]], R=[[[r]]], X0=[[[x0]]])
    X, K, F = tr.run(m, 7)
    for t in range(7):
        s = r + b * b * x
        k, f = b * x * a / s, b * x / s
        assert abs(K[t, 0, 0, 0] - k) <= 4e-16 * abs(k) and abs(F[t, 0, 0, 0] - f) <= 4e-16 * abs(f)
        x = a * a * x - a * x * b * k + q
        assert abs(X[t + 1, 0, 0, 0] - x) <= 1e-15 * x
    assert abs(X[7, 0, 0, 0] - rr.scalar_root(a, b, q, r)) <= 1e-3      # (and on its way to the root of the algebraic equation)


@pytest.mark.parametrize('name', tr.CASES)
def test_autograd_against_central_differences(name):
    T = 7
    m = tr.make(name, T, 'AB')
    G_X, G_K = tr.seeds(name, T, *m['B'].shape[-2:])
    worst = 0.0
    for gf in (0, 1):
        g = tr.gradients(m, T, G_X, G_K, gf)
        worst = max(worst, tr.fd_directional(m, T, G_X, G_K, gf, g))
    print('%-24s autograd against central differences: %.1e' % (name, worst))
    assert worst <= rr.FD_BOUND


def _schedule(hold, nent=4, Bt=2):
    """A cart-pole schedule: per entry and instance a perturbed model, with C, Qn, Rn, P0 and one realisation of measurements and inputs."""
    A0, Ct, Qn, Rn = rr.case('kalman_dual_cart_pole')
    rng = np.random.default_rng(5 + hold)
    A_traj = np.stack([np.stack([A0.T * (1 + 0.02 * rng.uniform(-1, 1, A0.shape)) for _ in range(Bt)]) for _ in range(nent)])
    Bm = rng.standard_normal((4, 1)) * 0.1
    P0 = rr._spd(rng, 4, lo=0.05)
    K = nent * hold
    return A_traj, Bm, Ct.T.copy(), Qn, Rn, P0, rng.standard_normal((K, Bt, 2)), rng.standard_normal((K, Bt, 1)), rng.standard_normal((Bt, 4))


@pytest.mark.parametrize('hold', [1, 3])
def test_the_loops_estimator_with_these_gains_is_the_textbook_kalman_filter(hold):
    """pympc_amd.kalman.LinearStateEstimator stepped as the device loop steps it -- update with the measurement of step k, then predict under
    the entry in force, xhat_{k+1} = A_e (xhat_k + L_e (y_k - C xhat_k)) + B u_k -- with ``kalman_gain_traj``'s gains, against a covariance-form
    Kalman filter written out here: the same estimates to rounding with hold = 1 (entry e IS step k), and with a hold the gain of an entry is
    the textbook gain of the entry's first step."""
    from pympc_amd.kalman import LinearStateEstimator
    A_traj, Bm, C, Qn, Rn, P0, Y, U, xh0 = _schedule(hold)
    nent, Bt = A_traj.shape[:2]
    L_traj, P_traj = tr.kalman_gain_traj(A_traj, C, Qn, Rn, P0, hold)
    assert L_traj.shape == (nent, Bt, 4, 2) and P_traj.shape == (nent + 1, Bt, 4, 4)
    for b in range(Bt):
        est = LinearStateEstimator(xh0[b], A_traj[0, b], Bm, C, np.zeros((2, 1)), L_traj[0, b])
        x, P = xh0[b].copy(), P0.copy()                    # the textbook filter: x = x[k|k-1], P = P[k|k-1]
        for k in range(nent * hold):
            e = k // hold
            Lk = P @ C.T @ np.linalg.inv(C @ P @ C.T + Rn)
            if k % hold == 0:
                assert rr.rel(L_traj[e, b], Lk) <= 1e-12 and rr.rel(P_traj[e, b], P) <= 1e-12, (k, e)
            xf, Pf = x + Lk @ (Y[k, b] - C @ x), P - Lk @ C @ P            # measurement update
            x, P = A_traj[e, b] @ xf + Bm @ U[k, b], A_traj[e, b] @ Pf @ A_traj[e, b].T + Qn      # time update under the entry in force
            P = 0.5 * (P + P.T)
            if hold == 1:
                est.A, est.L = A_traj[e, b], L_traj[e, b]
                est.update(Y[k, b])
                est.predict(U[k, b])
                assert np.abs(est.x - x).max() <= 1e-12 * max(1.0, np.abs(x).max()), k
        assert rr.rel(P_traj[nent, b], P) <= 1e-12


def test_lqr_traj_is_the_cost_of_its_own_closed_loop():
    T, Bt = 6, 2
    A, B, Q, R = rr.case('random_5_3')
    rng = np.random.default_rng(9)
    Ad = np.stack([np.stack([A * (1 + 0.05 * rng.uniform(-1, 1, A.shape)) for _ in range(Bt)]) for _ in range(T)])
    Bd = np.stack([np.stack([B * (1 + 0.05 * rng.uniform(-1, 1, B.shape)) for _ in range(Bt)]) for _ in range(T)])
    QxN = rr._spd(rng, 5)
    P_traj, K_traj = tr.lqr_traj(Ad, Bd, Q, R, QxN)
    assert P_traj.shape == (T + 1, Bt, 5, 5) and K_traj.shape == (T, Bt, 3, 5)
    for b in range(Bt):
        assert np.array_equal(P_traj[T, b], 0.5 * (QxN + QxN.T))
        x0 = rng.standard_normal(5)
        for start in (0, 2):                               # the cost-to-go from step `start`
            x, cost = x0.copy(), 0.0
            for t in range(start, T):
                u = -K_traj[t, b] @ x
                cost += x @ Q @ x + u @ R @ u
                x = Ad[t, b] @ x + Bd[t, b] @ u
            cost += x @ QxN @ x
            assert abs(cost - x0 @ P_traj[start, b] @ x0) <= 1e-12 * cost, (b, start)


def test_shape_and_gain_form_errors_come_before_any_library_call(monkeypatch):
    from pympc_amd import _lib, riccati
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('the library was asked for'))
    I2, b, r = np.eye(2), np.ones((2, 1)), np.eye(1)
    At = np.stack([I2] * 3)
    with pytest.raises(ValueError, match='gain_form'):
        riccati.dre(At, b, I2, r, I2, gain_form=2)
    with pytest.raises(ValueError, match='give the number of steps'):
        riccati.dre(I2, b, I2, r, I2)
    with pytest.raises(ValueError, match='disagree'):
        riccati.dre(At, np.stack([b] * 4), I2, r, I2)
    with pytest.raises(ValueError, match='T = 5'):
        riccati.dre(At, b, I2, r, I2, T=5)
    with pytest.raises(ValueError, match='X0 has shape'):
        riccati.dre(At, b, I2, r, np.eye(3))
    with pytest.raises(ValueError, match='batch size'):
        riccati.dre(np.stack([At] * 2, axis=1), b, np.stack([I2] * 3), r, I2)
    with pytest.raises(ValueError, match='seed'):
        riccati.dre_adjoint(At, b, I2, r, I2, np.stack([I2] * 4))
    with pytest.raises(ValueError, match='G_X has shape'):
        riccati.dre_adjoint(At, b, I2, r, I2, np.stack([I2] * 4), G_X=np.stack([I2] * 3))
    with pytest.raises(ValueError, match='want'):
        riccati.dre_adjoint(At, b, I2, r, I2, np.stack([I2] * 4), G_X=np.stack([I2] * 4), want=('S',))
    with pytest.raises(ValueError, match='hold'):
        riccati.kalman_gain_traj(At, b.T, I2, r, I2, hold=0)
    with pytest.raises(ValueError, match='A_traj'):
        riccati.kalman_gain_traj(I2, b.T, I2, r, I2)
    with pytest.raises(ValueError, match='Bd_traj'):
        riccati.lqr_traj(At, b, I2, r, I2)


def test_the_cpu_twin_has_no_riccati_difference_equation(twin):
    from pympc_amd import _lib, riccati
    assert not _lib.has_riccati_traj(twin)
    assert not any(hasattr(twin, s) for s in _lib.RICCATI_TRAJ_SYMBOLS)
    I2, b, r = np.eye(2), np.ones((2, 1)), np.eye(1)
    At = np.stack([I2] * 3)
    for call in (lambda: riccati.dre(At, b, I2, r, I2), lambda: riccati.dre(I2, b, I2, r, I2, T=2),
                 lambda: riccati.dre_adjoint(At, b, I2, r, I2, np.stack([I2] * 4), G_X=np.stack([I2] * 4)),
                 lambda: riccati.kalman_gain_traj(At, b.T, I2, r, I2), lambda: riccati.lqr_traj(At, np.stack([b] * 3), I2, r, I2)):
        with pytest.raises(NotImplementedError, match='mpcqp_dre'):
            call()
