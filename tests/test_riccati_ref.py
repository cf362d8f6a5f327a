"""tests/riccati_ref.py -- the numpy restatement of the Riccati kernels (pympc_amd/csrc/mpcqp_riccati.h) -- against scipy: the solution and
both gain forms against scipy.linalg.solve_discrete_are, its adjoint against central differences of scipy (h = 1e-6; symmetric
perturbations for Q and R, both gain forms seeded).  What it measures here, e_ref(case), is what the device's bounds are made of
(riccati_ref.E_REF, RES_REF, E_REF_ADJ: the recorded figures, which this test holds the restatement to).  No GPU needed.  Run with -s for the figures."""
import numpy as np
import pytest

import riccati_ref as rr

# the distance is scipy's error as much as the restatement's and moves with the BLAS build: the restatement is held to ten times its
# recorded distance (a tenth of the factor the device gets), and to 1e-13 where the record is smaller than that
SLACK, SCIPY_FLOOR = 10.0, 1e-13


@pytest.mark.parametrize('name', sorted(rr.CASES))
def test_solution_and_gains_against_scipy(name):
    e, r = [0.0, 0.0, 0.0], 0.0
    for A, B, Q, R in rr.copies(name):
        for gf in (0, 1):
            X, K, st, it, res = rr.dare(A, B, Q, R, gf)
            assert st == 1 and 1 <= it <= 20, (st, it)
            Xs, Ks = rr.scipy_dare(A, B, Q, R, gf)
            e[0], e[1 + gf], r = max(e[0], rr.rel(X, Xs)), max(e[1 + gf], rr.rel(K, Ks)), max(r, res)
            assert np.array_equal(X, X.T)
    print('%-28s e_ref X %.1e  K %.1e  F %.1e   res %.1e   steps %d' % (name, e[0], e[1], e[2], r, it))
    for k in range(3):
        assert e[k] <= max(SLACK * rr.E_REF[name][k], SCIPY_FLOOR), (k, e, rr.E_REF[name])
    assert r <= max(SLACK * rr.RES_REF[name], rr.RES_FLOOR), (r, rr.RES_REF[name])


def test_scalar_against_the_closed_form_root():
    a, b, q, r = (M[0, 0] for M in rr.SCALAR)
    X, K, st, it, res = rr.dare(*rr.SCALAR)
    root = rr.scalar_root(a, b, q, r)
    assert st == 1 and abs(X[0, 0] - root) <= 4e-16 * root
    assert abs(K[0, 0] - b * root * a / (r + b * b * root)) <= 1e-15


@pytest.mark.parametrize('name', sorted(rr.CASES))
def test_adjoint_against_central_differences_of_scipy(name):
    A, B, Q, R = rr.case(name)
    n, m = B.shape
    G_X, G_K = rr.seeds(name, n, m)
    worst = 0.0
    for gf in (0, 1):
        X, K, st, _, _ = rr.dare(A, B, Q, R, gf)
        g = rr.dare_adjoint(A, B, Q, R, X, K, G_X, G_K, gf)
        assert np.array_equal(g[2], g[2].T) and np.array_equal(g[3], g[3].T)
        worst = max(worst, rr.fd_directional(A, B, Q, R, G_X, G_K, gf, g[:4]))
        if n * m <= 8:                                     # every entry, where that is quick
            fd = rr.fd_loss_gradients(A, B, Q, R, G_X, G_K, gf)
            for a, f in zip(g[:4], fd):
                assert rr.rel(a, f) <= rr.FD_BOUND, (gf, rr.rel(a, f))
    print('%-28s adjoint against central differences: %.1e' % (name, worst))
    assert worst <= rr.FD_BOUND                             # (riccati_ref.E_REF_ADJ records the figure: finite-difference noise, 3e-10 .. 3e-7)


def test_outcomes_that_are_not_solutions():
    A, B, Q, R = rr.case(rr.NOT_PD)
    X, K, st, it, res = rr.dare(A, B, Q, R)
    assert (st, it, res) == (-1, 0, 0.0) and not X.any() and not K.any()
    # an uncontrollable unstable mode: the iterate overflows after eleven doublings; under a smaller budget the budget ends it
    bad = (np.diag([1.2, 0.5]), np.array([[0.0], [1.0]]), np.eye(2), np.eye(1))
    X, K, st, it, res = rr.dare(*bad)
    assert st == 0 and it <= rr.MAX_ITER and not X.any() and not K.any() and res == 0.0
    assert rr.dare(*bad, max_iter=8)[2:4] == (0, 8)
