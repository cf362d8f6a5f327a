"""Recovering a physical parameter of the plant from an expert's closed-loop inputs, THROUGH a controller that tracks the plant's TRUE
linearisations (pympc_amd.torch_layer.mpc_rollout_affine).

examples/learn_plant_parameter_through_ltv_mpc.py has to freeze the angle-dependent factors of the cart pole, because a proper linearisation
away from the equilibrium has an offset, x+ = A_e x + B_e u + c_e with c_e = f(xbar_e, ubar_e) - A_e xbar_e - B_e ubar_e, and its rollout could
not carry one.  This is the same experiment with the true linearisation: (A_e, B_e, c_e) are the Jacobians and the offset of the nonlinear
step f at a sequence of operating points (the pendulum at rest at an angle), torch functions of the pendulum length l by torch.func.  The
schedule is the controller's model AND the plant: ``offset_in_plant=True`` gives the plant the offset too.  An expert that knows the true
length regulates a batch of pendulums; a learner starts from a wrong length and descends

    loss(l) = mean_i sum_k |u_k(x0_i; l) - u_k^expert(x0_i)|^2

by the same rule as the other example (a step is halved until the loss falls by a quarter of what the gradient predicts, doubled after a step
that needed no halving).  Forward is ONE taped device loop (mpcqp_rollout_affine); backward ONE mpcqp_rollout_adjoint_affine call
(include_ext5/mpcqp_rollout_affine.h), which returns the gradient of every schedule entry's A_e, B_e and c_e; torch chains those into l.

    python examples/learn_plant_parameter_through_ltv_affine_mpc.py [--batch 64] [--steps 12] [--hold 3] [--iters 12] [--eps 1e-8] [--step 2e-3]
    (small, for a test: --batch 16 --steps 12 --iters 8)
"""
import argparse
import os
import sys

import numpy as np
import torch
from torch.func import jacrev, vmap

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pympc_amd import BatchMPCController, fixtures            # noqa: E402
from pympc_amd.torch_layer import mpc_rollout_affine          # noqa: E402

M, m, b, ft, g, Ts = 0.5, 0.2, 0.1, 0.1, 9.81, 50e-3           # examples/example_inverted_pendulum.py:10-17 (l = 0.3 there)
ARMIJO = 0.25


def step(x, u, l):
    """The nonlinear pendulum on a cart, one forward-Euler step (plant() of examples/closed_loop_ltv.py), in torch: x [4], u [1], l 0-d."""
    F, v, th, om = u[0], x[1], x[2], x[3]
    s, c = torch.sin(th), torch.cos(th)
    den = M + m * (1.0 - c * c)
    acc = (m * l * s * om ** 2 - m * g * s * c + m * ft * c * om + F - b * v) / den
    alp = ((M + m) * (g * s - ft * om) - m * l * om ** 2 * s * c - (F - b * v) * c) / (l * den)
    return x + Ts * torch.stack([v, acc, om, alp])


def schedule(l, theta):
    """(A [nseg, B, 4, 4], B [nseg, B, 4, 1], c [nseg, B, 4]) of the step with length ``l`` linearised at the operating points (0, 0, theta, 0),
    u = 0, ``theta`` [nseg, B]: the true Jacobians and the offset c = f(xbar, 0) - A xbar."""
    z = torch.zeros_like(theta)
    xbar = torch.stack([z, z, theta, z], dim=-1).reshape(-1, 4)
    ubar = torch.zeros((xbar.shape[0], 1), dtype=theta.dtype, device=theta.device)
    A, Bm = vmap(jacrev(step, argnums=(0, 1)), in_dims=(0, 0, None))(xbar, ubar, l)
    f0 = vmap(step, in_dims=(0, 0, None))(xbar, ubar, l)
    c = f0 - torch.einsum('eij,ej->ei', A, xbar)
    shp = tuple(theta.shape)
    return A.reshape(shp + (4, 4)), Bm.reshape(shp + (4, 1)), c.reshape(shp + (4,))


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
    ap = argparse.ArgumentParser(description='Learn the pendulum length through an MPC controller that tracks true linearisations with their offset.')
    ap.add_argument('--batch', type=int, default=64, help='pendulums (16 is enough for a quick run)')
    ap.add_argument('--steps', type=int, default=12, help='closed-loop steps of a rollout')
    ap.add_argument('--hold', type=int, default=3, help='steps a linearisation is held for')
    ap.add_argument('--iters', type=int, default=12, help='descent iterations (8 is enough for a quick run)')
    ap.add_argument('--eps', type=float, default=1e-8, help='eps_abs = eps_rel of the solves')
    ap.add_argument('--step', type=float, default=2e-3, help='first step length')
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
        At, Bt, ct = schedule(l, theta)
        # (the first solve is made under what the controller holds when the loop begins: entry 0's model through params, its offset through d0)
        return mpc_rollout_affine(K, x0, a.steps, ct, d_hold=a.hold, d0=ct[0], Ad_traj=At, Bd_traj=Bt, hold=a.hold, u_prev=um1,
                                  params=dict(Ad=At[0], Bd=Bt[0]), offset_in_plant=True)

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
    step_len, ratio, halvings = a.step, float('nan'), 0
    loss = loss_of(l)
    for it in range(a.iters + 1):
        print('iteration %2d: loss %.10e   step %.3g   length %.6f   decrease / predicted %.4f   halvings %d' % (it, loss.item(), step_len, l.item(), ratio, halvings))
        if it == a.iters:
            break
        grad, = torch.autograd.grad(loss, [l])
        g2 = float((grad * grad).item())
        halved = False
        while True:                                        # halve the step until the loss falls by a quarter of step |grad|^2
            trial = (l.detach() - step_len * grad).requires_grad_(True)
            new = loss_of(trial) if trial.item() > 0.05 else None
            ratio = (loss.item() - new.item()) / (step_len * g2) if new is not None and g2 > 0 else 0.0
            if ratio >= ARMIJO or step_len < 1e-12:
                break
            step_len *= 0.5; halvings += 1; halved = True
        if new is not None:
            l, loss = trial, new
        if not halved:
            step_len *= 2.0
    print('parameter: true %.6f start %.6f learned %.6f' % (true, start, l.item()))


if __name__ == '__main__':
    main()
