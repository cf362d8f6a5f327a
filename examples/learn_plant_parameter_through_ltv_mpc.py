"""Recovering a physical parameter of the plant from an expert's closed-loop inputs, THROUGH a controller that tracks relinearised models
(pympc_amd.torch_layer.mpc_rollout_tv).

The plant is the cart pole of examples/closed_loop_ltv.py: its equations with the angle-dependent factors frozen at a sequence of angles, one
model per ``hold`` steps -- a schedule (Ad_traj, Bd_traj) that is a torch function of the pendulum length l.  An expert
``BatchMPCController`` that knows the true length regulates a batch of pendulums from different initial angles; the schedule is the
controller's model AND the plant (``mpcqp_rollout_tv``: ``update_model`` between the steps of the device loop, the plant following the model
in force).  A learner starts from a wrong length and descends

    loss(l) = mean_i sum_k |u_k(x0_i; l) - u_k^expert(x0_i)|^2

by plain gradient descent.  Forward is ONE taped device loop under the schedule; backward ONE ``mpcqp_rollout_adjoint_tv`` call
(include_ext/mpcqp_rollout_tv.h): a reverse sweep over the tape that reads every entry's model and scaling from the slot it was solved
under, and returns the gradient of every schedule entry -- through the solves made under it and through the plant steps it was in force --
summed over the batch on the device.  torch chains those into l.  Nothing of a training step leaves the GPU but the loss that is printed.
The closed loop is piecewise smooth in l: a step is halved until the loss falls by a quarter of what the gradient predicts (the rule of
examples/differentiable_mpc.py), and doubled again after a step that needed no halving.

    python examples/learn_plant_parameter_through_ltv_mpc.py [--batch 64] [--steps 12] [--hold 3] [--iters 12] [--eps 1e-8] [--step 2e-3]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pympc_amd import BatchMPCController, fixtures            # noqa: E402
from pympc_amd.torch_layer import mpc_rollout_tv              # noqa: E402

M, m, b, ft, g, Ts = 0.5, 0.2, 0.1, 0.1, 9.81, 50e-3           # examples/example_inverted_pendulum.py:10-17 (l = 0.3 there)
ARMIJO = 0.25


def schedule(l, theta):
    """(Ad_traj [nseg, B, 4, 4], Bd_traj [nseg, B, 4, 1]) of the cart pole with length ``l`` (a 0-d tensor) linearised at the angles
    ``theta`` [nseg, B] at rest: model_at of examples/closed_loop_ltv.py, in torch."""
    s, c = torch.sin(theta), torch.cos(theta)
    sinc = torch.where(theta.abs() > 1e-12, s / theta, torch.ones_like(theta))
    den = M + m * (1.0 - c * c)
    o, z = torch.ones_like(theta), torch.zeros_like(theta)
    Ac = torch.stack([torch.stack([z, o, z, z], dim=-1),
                      torch.stack([z, -b / den, -m * g * c * sinc / den, m * ft * c / den], dim=-1),
                      torch.stack([z, z, z, o], dim=-1),
                      torch.stack([z, b * c / (l * den), (M + m) * g * sinc / (l * den), -(M + m) * ft / (l * den)], dim=-1)], dim=-2)
    Bc = torch.stack([z, 1.0 / den, z, -c / (l * den)], dim=-1).unsqueeze(-1)
    return torch.eye(4, dtype=theta.dtype, device=theta.device) + Ts * Ac, Ts * Bc


def controller(kw, X0, eps):
    B = X0.shape[0]
    st = lambda a: np.broadcast_to(np.asarray(a, dtype=float), (B,) + np.shape(a))
    K = BatchMPCController(st(kw['Ad']), st(kw['Bd']), Np=kw['Np'], x0=X0, xref=st(kw['xref']), uref=st(kw['uref']), uminus1=st(kw['uminus1']),
                           Qx=st(kw['Qx']), QxN=st(kw['QxN']), Qu=st(kw['Qu']), QDu=st(kw['QDu']), xmin=st(kw['xmin']), xmax=st(kw['xmax']),
                           umin=st(kw['umin']), umax=st(kw['umax']), Dumin=st(kw['Dumin']), Dumax=st(kw['Dumax']), eps_feas=kw['eps_feas'],
                           eps_abs=eps, eps_rel=eps, max_iter=200000)
    K.setup(solve=False)
    return K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64); ap.add_argument('--steps', type=int, default=12); ap.add_argument('--hold', type=int, default=3)
    ap.add_argument('--iters', type=int, default=12); ap.add_argument('--eps', type=float, default=1e-8); ap.add_argument('--step', type=float, default=2e-3)
    a = ap.parse_args()
    kw = fixtures.cart_pole()
    true, start = 0.3, 0.4                                 # the pendulum's length, and the learner's first guess
    nseg = (a.steps + a.hold - 1) // a.hold
    rng = np.random.default_rng(0)
    th0 = np.deg2rad(rng.uniform(8.0, 22.0, a.batch))
    X0 = np.stack([np.zeros(a.batch), np.zeros(a.batch), th0, np.zeros(a.batch)], axis=1)
    dev = torch.device('cuda:0')
    t = lambda v: torch.tensor(np.asarray(v, dtype=float), dtype=torch.float64, device=dev)
    x0, um1 = t(X0), t(np.zeros((a.batch, 1)))          # (every rollout starts from the same state and the same previous input)
    theta = t(th0[None, :] * 0.6 ** np.arange(nseg)[:, None])      # the angles the loop is relinearised at: the regulated pendulum comes upright

    def rollout(K, l):
        Adt, Bdt = schedule(l, theta)
        # (the first solve is made under the model the controller holds when the loop begins: entry 0's, through params)
        return mpc_rollout_tv(K, x0, a.steps, Adt, Bdt, a.hold, u_prev=um1, params=dict(Ad=Adt[0], Bd=Bdt[0]))

    expert = controller(kw, X0, a.eps)
    with torch.no_grad():
        _, U_exp = rollout(expert, t(true))
    expert.prob.rollout_adjoint(g_u=torch.ones_like(U_exp), want=('lam',))      # (one sweep of the expert's tape: how often its active set or its model changes)
    _, _, st, nfac = expert.prob.rollout_info()
    assert np.all(st == 1), 'an expert step did not end solved'
    print('expert: length %.3f, %d instances, %d steps, %d schedule entries; factorizations per step %.3f'
          % (true, a.batch, a.steps, nseg, nfac.sum() / float(a.batch * a.steps)))

    learner = controller(kw, X0, a.eps)
    loss_of = lambda l: ((rollout(learner, l)[1] - U_exp) ** 2).sum(dim=(0, 2)).mean()
    l = t(start).requires_grad_(True)
    step, ratio, halvings = a.step, float('nan'), 0
    loss = loss_of(l)
    for it in range(a.iters + 1):
        print('iteration %2d: loss %.10e   step %.3g   length %.6f   decrease / predicted %.4f   halvings %d' % (it, loss.item(), step, l.item(), ratio, halvings))
        if it == a.iters:
            break
        grad, = torch.autograd.grad(loss, [l])
        g2 = float((grad * grad).item())
        halved = False
        while True:                                        # halve the step until the loss falls by a quarter of step |grad|^2
            trial = (l.detach() - step * grad).requires_grad_(True)
            new = loss_of(trial) if trial.item() > 0.05 else None
            ratio = (loss.item() - new.item()) / (step * g2) if new is not None and g2 > 0 else 0.0
            if ratio >= ARMIJO or step < 1e-12:
                break
            step *= 0.5; halvings += 1; halved = True
        if new is not None:
            l, loss = trial, new
        if not halved:
            step *= 2.0
    print('parameter: true %.6f start %.6f learned %.6f' % (true, start, l.item()))


if __name__ == '__main__':
    main()
