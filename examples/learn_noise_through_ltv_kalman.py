"""Recovering the process-noise scale a Kalman filter was designed for from a recorded closed loop, THROUGH an output-feedback controller that
tracks relinearised models with the gains of the TIME-VARYING filter (pympc_amd.torch_layer.mpc_rollout_tv_est, kalman_gain_traj).

The plant is the relinearised cart pole of examples/learn_plant_parameter_through_ltv_mpc.py, one model per ``hold`` steps, but nobody measures
its full state: y = C x + v gives the cart's position and the pendulum's angle, and the controller sees the estimate of an observer that is
relinearised with it,

    xhat_{k+1} = A_e (xhat_k + L_e (y_k - C xhat_k)) + B_e u_k,        L = kalman_gain_traj(A, C, q^2 I, r^2 I, P0, hold)      (e = k // hold)

-- where examples/learn_noise_through_scheduled_observer.py designs one STATIONARY filter per entry, here the covariance is carried from step
to step, P_{k+1} = A_e (P_k - L_k C P_k) A_e' + q^2 I from the covariance P0 of the first estimate, and entry e gets the gain of its first
step: the Kalman filter of the time-varying system, a torch function of the process-noise scale q the designer assumed
(``pympc_amd.torch_layer.kalman_gain_traj``: one batched Riccati recursion on the device, with its adjoint).  A reference loop whose observer was designed for the true q is recorded: its
inputs and its estimates, under one realisation of the disturbances w, v and from a wrong first estimate.  A learner starts from a q four
times too large and descends the closed-loop cost

    loss(q) = mean_i sum_k |u_k(q) - u_k^rec|^2 + |xhat_k(q) - xhat_k^rec|^2

under the same realisation, by plain gradient descent in log q.  Forward is ONE taped device loop under the schedule of models and gains
(mpcqp_rollout_tv_est); backward ONE mpcqp_rollout_adjoint_tv_est (include_ext2/mpcqp_rollout_tv_est.h): a reverse sweep that returns the
gradient of every gain entry, which torch chains through ONE adjoint recursion (mpcqp_dre_adjoint) down to q.  Nothing of a training step leaves the
GPU but the loss that is printed.  The step rule is that of examples/learn_plant_parameter_through_ltv_mpc.py: halved until the loss falls by
a quarter of what the gradient predicts, doubled after a step that needed no halving; the first trial moves log q by ``--step``.

    python examples/learn_noise_through_ltv_kalman.py [--batch 64] [--steps 12] [--hold 3] [--iters 12] [--eps 1e-8] [--step 1.0]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pympc_amd import fixtures                                 # noqa: E402
from pympc_amd.torch_layer import mpc_rollout_tv_est, kalman_gain_traj      # noqa: E402
from learn_plant_parameter_through_ltv_mpc import schedule, controller, ARMIJO      # noqa: E402

LENGTH = 0.3               # the pendulum's length (known here)
Q_TRUE, Q_START, R = 0.005, 0.02, 0.005      # the process-noise scale: the plant's and the learner's first guess; the measurement-noise scale
SIGMA0 = 0.02              # the standard deviation of the first estimate's error: P0 = SIGMA0^2 I


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64); ap.add_argument('--steps', type=int, default=12); ap.add_argument('--hold', type=int, default=3)
    ap.add_argument('--iters', type=int, default=12); ap.add_argument('--eps', type=float, default=1e-8); ap.add_argument('--step', type=float, default=1.0)
    a = ap.parse_args()
    kw = fixtures.cart_pole()
    B, K = a.batch, a.steps
    nseg = (K + a.hold - 1) // a.hold
    rng = np.random.default_rng(0)
    th0 = np.deg2rad(rng.uniform(8.0, 22.0, B))
    X0 = np.stack([np.zeros(B), np.zeros(B), th0, np.zeros(B)], axis=1)
    XH0 = X0 + SIGMA0 * rng.standard_normal(X0.shape)            # the observer starts from a wrong estimate: its gain matters from the first step
    dev = torch.device('cuda:0')
    t = lambda v: torch.tensor(np.asarray(v, dtype=float), dtype=torch.float64, device=dev)
    x0, xh0, um1 = t(X0), t(XH0), t(np.zeros((B, 1)))
    w, v = t(Q_TRUE * rng.standard_normal((K, B, 4))), t(R * rng.standard_normal((K, B, 2)))      # ONE realisation, the same for every rollout
    theta = t(th0[None, :] * 0.6 ** np.arange(nseg)[:, None])
    Cm = t([[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])
    Adt, Bdt = schedule(t(LENGTH), theta)
    eye4, Rn = torch.eye(4, dtype=torch.float64, device=dev), R * R * torch.eye(2, dtype=torch.float64, device=dev)

    def gains(logq):
        """L [nseg, B, 4, 2]: the time-varying Kalman filter's gain at every entry's first step for the process noise exp(logq)^2 I."""
        L, P = kalman_gain_traj(Adt, Cm, torch.exp(2.0 * logq) * eye4, Rn, SIGMA0 * SIGMA0 * eye4, hold=a.hold)
        assert bool((L.status == 1).all()), 'a Riccati recursion did not run through'
        return L

    def rollout(Kc, logq):
        # (the first solve is made under the model the controller holds when the loop begins: entry 0's, through params)
        return mpc_rollout_tv_est(Kc, x0, xh0, K, Adt, Bdt, a.hold, Cm, L_traj=gains(logq), v=v, u_prev=um1, w=w, params=dict(Ad=Adt[0], Bd=Bdt[0]))

    ref = controller(kw, XH0, a.eps)
    with torch.no_grad():
        _, XH_rec, _, U_rec = rollout(ref, t(math.log(Q_TRUE)))
    ref.prob.rollout_adjoint(g_u=torch.ones_like(U_rec), want=('lam',))      # (one sweep of the recorded loop's tape: how often its active set or its model changes)
    _, _, st, nfac = ref.prob.rollout_info()
    assert np.all(st == 1), 'a step of the recorded loop did not end solved'
    print('recorded: noise scale %.4f, %d instances, %d steps, %d schedule entries; factorizations per step %.3f'
          % (Q_TRUE, B, K, nseg, nfac.sum() / float(B * K)))

    learner = controller(kw, XH0, a.eps)

    def loss_of(logq):
        _, XH, _, U = rollout(learner, logq)
        return (((U - U_rec) ** 2).sum(dim=(0, 2)) + ((XH - XH_rec) ** 2).sum(dim=(0, 2))).mean()
    p = t(math.log(Q_START)).requires_grad_(True)
    step, ratio, halvings = None, float('nan'), 0
    loss = loss_of(p)
    loss0 = loss.item()
    for it in range(a.iters + 1):
        print('iteration %2d: loss %.10e   step %.3g   noise scale %.6f   decrease / predicted %.4f   halvings %d'
              % (it, loss.item(), float('nan') if step is None else step, math.exp(p.item()), ratio, halvings))
        if it == a.iters:
            break
        grad, = torch.autograd.grad(loss, [p])
        g2 = float((grad * grad).item())
        if g2 == 0.0:
            break
        if step is None:
            step = a.step / math.sqrt(g2)
        halved = False
        while True:                                        # halve the step until the loss falls by a quarter of step |grad|^2
            trial = (p.detach() - step * grad).requires_grad_(True)
            new = loss_of(trial)
            ratio = (loss.item() - new.item()) / (step * g2)
            if ratio >= ARMIJO or step < 1e-14:
                break
            step *= 0.5; halvings += 1; halved = True
        if ratio >= ARMIJO:
            p, loss = trial, new
        if not halved:
            step *= 2.0
    print('parameter: true %.6f start %.6f learned %.6f' % (Q_TRUE, Q_START, math.exp(p.item())))
    print('LTV_KALMAN_OK loss0 %.10e loss1 %.10e q %.6f' % (loss0, loss.item(), math.exp(p.item())))


if __name__ == '__main__':
    main()
