"""GPU tests of the closed loop's carry inside the latency round (admm_latw / latw_carry, mpcqp_latw.h and mpcqp_latw_check.h): a solve that
converges in the round's own termination test moves on to the next step of its queue item -- output, plant, update, q, warm start from the
owner registers -- without leaving the function.  MPCQP_TUNE_NO_CARRY leaves the round after every solve (write-back, begin, prologue), the
path every step took before.  The two must agree bit for bit: trajectories, statuses, iteration counts, the handle's final iterate and record.
Run on the GPU box with:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest

from util import carry_on_and_off

pytestmark = pytest.mark.gpu


def test_carry_headline_batch_persistent_queue():
    """1024 x (12,4,30) for 20 steps: the headline's kernel, persistent launch with step-range parts."""
    from pympc_amd import fixtures
    B, steps = 1024, 20
    kws = [fixtures.random_lti(i) for i in range(B)]
    w = 0.01 * np.random.default_rng(3).standard_normal((steps, B, 12))
    a, (carried, back, parts) = carry_on_and_off(kws, steps, w=w)
    assert (a['status'] == 1).mean() > 0.9
    assert parts == 4                                     # (8 / 6 / 4 / 2 steps: 256 resident slots, 16 items each)
    assert carried > 0.5 * B * (steps - parts) and back == 0, (carried, back)


def test_carry_small_batch_two_launches():
    """7 instances (one workgroup each, not persistent), two consecutive launches of 9 steps."""
    from pympc_amd import fixtures
    kws = [fixtures.random_lti(300 + i) for i in range(7)]
    w = 0.01 * np.random.default_rng(4).standard_normal((18, 7, 12))
    _, (carried, back, parts) = carry_on_and_off(kws, 9, nruns=2, w=w)
    assert parts == 0 and carried > 0 and back == 0, (carried, back, parts)


def test_carry_falls_back_at_iteration_limit():
    """max_iter below convergence: no solve ends in the round's own test, output() falls back to u_failure = uref every step."""
    from pympc_amd import fixtures
    kws = [fixtures.random_lti(500 + i) for i in range(7)]
    for kw in kws:
        kw['uref'] = np.array([0.05, -0.02, 0.01, 0.03])
    a, (carried, back, _) = carry_on_and_off(kws, 6, max_iter=30)
    assert (a['status'] != 1).any()
    assert carried <= (a['status'][:-1] == 1).sum() and back == 0      # (only a step after a solved one can be carried into)


def test_carry_with_rho_updates_mid_solve():
    """eps 1e-9: long solves whose rounds also end in rho estimates (the generic check), mixed with carried steps."""
    from pympc_amd import fixtures
    kws = [fixtures.random_lti(700 + i) for i in range(7)]
    w = 0.01 * np.random.default_rng(5).standard_normal((8, 7, 12))
    a, (carried, back, _) = carry_on_and_off(kws, 8, w=w, eps_abs=1e-9, eps_rel=1e-9, max_iter=20000)
    assert (a['status'] == 1).all()
    assert carried > 0 and back == 0


def test_carry_around_an_infeasible_step():
    """Instances whose first QP is primal infeasible (u_{-1} far outside what the bounds allow) beside feasible ones."""
    from pympc_amd import fixtures
    kws = [fixtures.random_lti(600 + i) for i in range(7)]
    kws[1]['uminus1'] = np.array([5.0, 0.0, 0.0, 0.0])
    kws[4]['uminus1'] = np.array([0.0, -7.0, 0.0, 0.0])
    a, (carried, _, _) = carry_on_and_off(kws, 6)
    assert carried > 0
    assert np.array_equal(a['u'][0, 1], kws[1]['uref']) and np.array_equal(a['u'][0, 4], kws[4]['uref'])      # (u_failure after setup's solve)


def test_carry_off_with_a_moving_reference():
    """A reference trajectory: the round never carries (q changes everywhere), the loop is unchanged."""
    from pympc_amd import fixtures
    B, steps = 7, 6
    kws = [fixtures.random_lti(800 + i) for i in range(B)]
    xref = np.zeros((steps, B, 12)); xref[:, :, 0] = 0.05 * np.arange(steps)[:, None]
    _, (carried, _, _) = carry_on_and_off(kws, steps, run_kw=lambda i: dict(xref_traj=xref))
    assert carried == 0


def test_carry_off_with_output_feedback():
    """An estimator in the loop (ny > 0): the round never carries, the loop is unchanged."""
    from pympc_amd import fixtures
    from pympc_amd.kalman import BatchLinearStateEstimator
    B, steps = 7, 6
    kws = [fixtures.random_lti(900 + i) for i in range(B)]
    st = lambda k: np.stack([np.asarray(d[k], dtype=float) for d in kws])
    C = np.tile(np.eye(12)[:3], (B, 1, 1))
    Lg = np.tile(0.3 * np.eye(12)[:, :3], (B, 1, 1))
    v = 1e-3 * np.random.default_rng(6).standard_normal((steps, B, 3))

    def run_kw(i):
        return dict(estimator=BatchLinearStateEstimator(st('x0'), st('Ad'), st('Bd'), C, Lg, x_true=st('x0').copy(), v=v))
    _, (carried, _, _) = carry_on_and_off(kws, steps, run_kw=run_kw)
    assert carried == 0


def test_carry_hands_back_when_a_row_type_changes():
    """A plant state that stops being finite (a NaN disturbance into one instance's step 3): stage 0's dynamics rows, equalities while -x0 is
    finite, stop being equalities.  latw_carry has already made that step's transition inside the round; it hands the step back, the kernel
    runs its begin (new types, refactorization) and the loop goes on exactly as without the carry."""
    from pympc_amd import fixtures
    B, steps = 7, 6
    kws = [fixtures.random_lti(1100 + i) for i in range(B)]
    w = 0.01 * np.random.default_rng(7).standard_normal((steps, B, 12))
    w[3, 2, 0] = np.nan
    a, (carried, back, _) = carry_on_and_off(kws, steps, w=w, max_iter=2000)
    assert back >= 1 and carried > back, (carried, back)
    assert np.isnan(a['x'][4, 2]).any() and np.isfinite(a['x'][:, [0, 1, 3, 4, 5, 6]]).all()
