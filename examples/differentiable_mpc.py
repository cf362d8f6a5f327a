"""Tuning a reference by gradient descent THROUGH the controller (pympc_amd.torch_layer.mpc_step).

256 copies of one (nx, nu, Np) = (12, 4, 30) controller start from 256 different states.  A constant reference xref, shared by all of them,
is tuned so that a three-step closed-loop rollout

    u_k = K(x_k, u_{k-1}, xref),   x_{k+1} = Ad x_k + Bd u_k,   k = 0, 1, 2

lands on a target state: loss = mean_i |x_3^(i) - target|^2.  Forward is three batched MPC solves on the device; backward is three
mpcqp_adjoint calls (one active-set KKT factorization per instance and step) chained by torch.autograd through the plant.  The adjoint
differentiates the solution a controller holds NOW, so the rollout uses one controller per step.  The control law is piecewise affine
in xref, the loss piecewise quadratic: plain gradient descent with an Armijo step.  A step is taken only if the loss falls by at least a
quarter of what the gradient predicts to first order, step |grad|^2 -- a test of the gradient itself, which a merely downhill direction or
a wrongly scaled one does not pass -- and is halved otherwise; every line prints the ratio of the actual to the predicted decrease, which
is 1 - O(step) for a correct gradient.

    python examples/differentiable_mpc.py [--batch 256] [--iters 12] [--eps 1e-8] [--step 0.1]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pympc_amd import BatchMPCController, fixtures            # noqa: E402
from pympc_amd.torch_layer import mpc_step                    # noqa: E402

STEPS = 3
ARMIJO = 0.25


def controllers(kw, X0, eps):
    B = X0.shape[0]
    st = lambda a: np.broadcast_to(np.asarray(a, dtype=float), (B,) + np.shape(a))
    Ks = []
    for _ in range(STEPS):
        K = BatchMPCController(st(kw['Ad']), st(kw['Bd']), Np=kw['Np'], x0=X0, xref=st(kw['xref']), uref=st(kw['uref']), uminus1=st(kw['uminus1']),
                               Qx=st(kw['Qx']), QxN=st(kw['QxN']), Qu=st(kw['Qu']), QDu=st(kw['QDu']), xmin=st(kw['xmin']), xmax=st(kw['xmax']),
                               umin=st(kw['umin']), umax=st(kw['umax']), Dumin=st(kw['Dumin']), Dumax=st(kw['Dumax']), eps_feas=kw['eps_feas'],
                               eps_abs=eps, eps_rel=eps, max_iter=200000)
        K.setup(solve=False)
        Ks.append(K)
    return Ks


def rollout_loss(Ks, Ad, Bd, x0, um1, xref, target):
    x, u = x0, um1
    xr = xref.expand(x0.shape[0], -1)
    for K in Ks:
        u = mpc_step(K, x, u, xr)
        x = x @ Ad.T + u @ Bd.T
    return ((x - target) ** 2).sum(dim=1).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256); ap.add_argument('--iters', type=int, default=12)
    ap.add_argument('--eps', type=float, default=1e-8); ap.add_argument('--step', type=float, default=0.1)
    a = ap.parse_args()
    kw = fixtures.random_lti(0)
    nx = kw['Ad'].shape[0]
    rng = np.random.default_rng(0)
    X0 = kw['x0'][None] * rng.uniform(0.2, 1.0, (a.batch, 1)) + 0.05 * rng.standard_normal((a.batch, nx))
    dev = torch.device('cuda:0')
    t = lambda v: torch.tensor(np.asarray(v, dtype=float), dtype=torch.float64, device=dev)
    Ad, Bd, x0, um1 = t(kw['Ad']), t(kw['Bd']), t(X0), t(np.zeros((a.batch, kw['Bd'].shape[1])))
    target = t(0.3 * np.ones(nx))
    Ks = controllers(kw, X0, a.eps)
    xref = torch.zeros(nx, dtype=torch.float64, device=dev, requires_grad=True)
    step, ratio, halvings = a.step, float('nan'), 0
    loss = rollout_loss(Ks, Ad, Bd, x0, um1, xref, target)
    for it in range(a.iters + 1):
        print('iteration %2d: loss %.10e   step %.3g   |xref| %.4f   decrease / predicted %.4f   halvings %d'
              % (it, loss.item(), step, xref.detach().norm().item(), ratio, halvings))
        if it == a.iters:
            break
        grad, = torch.autograd.grad(loss, xref)
        weak = sum(int(K.prob.adjoint_info()[1].sum()) for K in Ks)
        if weak:
            print('              (%d weakly active rows in the batch: one-sided gradients there)' % weak)
        g2 = float((grad * grad).sum().item())
        while True:                                        # Armijo: halve the step until the loss falls by a quarter of step |grad|^2
            trial = (xref.detach() - step * grad).requires_grad_(True)
            new = rollout_loss(Ks, Ad, Bd, x0, um1, trial, target)
            ratio = (loss.item() - new.item()) / (step * g2) if g2 > 0 else 0.0
            if ratio >= ARMIJO or step < 1e-12:
                break
            step *= 0.5; halvings += 1
        xref, loss = trial, new
    print('tuned xref:', np.array2string(xref.detach().cpu().numpy(), precision=4))


if __name__ == '__main__':
    main()
