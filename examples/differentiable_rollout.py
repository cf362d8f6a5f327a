"""Tuning a reference by gradient descent THROUGH a closed loop on ONE controller (pympc_amd.torch_layer.mpc_rollout).

The tuning problem of examples/differentiable_mpc.py over a longer horizon: 256 copies of one (nx, nu, Np) = (12, 4, 30) controller start
from 256 different states, and a constant reference xref, shared by all of them, is tuned so that a K-step closed-loop rollout

    u_k = K(x_k, u_{k-1}, xref),   x_{k+1} = Ad x_k + Bd u_k,   k = 0 .. K-1

lands on a target state: loss = mean_i |x_K^(i) - target|^2.  Forward is ONE controller rolled out by the device loop with a tape
(mpcqp_rollout); backward is ONE mpcqp_rollout_adjoint call -- a reverse sweep over the tape in a single kernel launch, which factors the
active-set KKT system of a step only where its active set differs from that of the step behind it (the line printed per iteration says how
many factorizations per step the sweep made).  Where examples/differentiable_mpc.py needs one controller, one setup and one factorization
per step, this needs one handle whatever K is.  The descent is the same: plain gradient descent with an Armijo step -- a step is taken
only if the loss falls by at least a quarter of what the gradient predicts to first order, which a wrong gradient does not pass.

    python examples/differentiable_rollout.py [--batch 256] [--steps 10] [--iters 12] [--eps 1e-8] [--step 0.1]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pympc_amd import BatchMPCController, fixtures            # noqa: E402
from pympc_amd.torch_layer import mpc_rollout                 # noqa: E402

ARMIJO = 0.25


def controller(kw, X0, eps):
    B = X0.shape[0]
    st = lambda a: np.broadcast_to(np.asarray(a, dtype=float), (B,) + np.shape(a))
    K = BatchMPCController(st(kw['Ad']), st(kw['Bd']), Np=kw['Np'], x0=X0, xref=st(kw['xref']), uref=st(kw['uref']), uminus1=st(kw['uminus1']),
                           Qx=st(kw['Qx']), QxN=st(kw['QxN']), Qu=st(kw['Qu']), QDu=st(kw['QDu']), xmin=st(kw['xmin']), xmax=st(kw['xmax']),
                           umin=st(kw['umin']), umax=st(kw['umax']), Dumin=st(kw['Dumin']), Dumax=st(kw['Dumax']), eps_feas=kw['eps_feas'],
                           eps_abs=eps, eps_rel=eps, max_iter=200000)
    K.setup(solve=False)
    return K


def rollout_loss(K, steps, x0, um1, xref, target):
    X, _ = mpc_rollout(K, x0, steps, u_prev=um1, xref=xref.expand(x0.shape[0], -1))
    return ((X[-1] - target) ** 2).sum(dim=1).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256); ap.add_argument('--steps', type=int, default=10); ap.add_argument('--iters', type=int, default=12)
    ap.add_argument('--eps', type=float, default=1e-8); ap.add_argument('--step', type=float, default=0.1)
    a = ap.parse_args()
    kw = fixtures.random_lti(0)
    nx = kw['Ad'].shape[0]
    rng = np.random.default_rng(0)
    X0 = kw['x0'][None] * rng.uniform(0.2, 1.0, (a.batch, 1)) + 0.05 * rng.standard_normal((a.batch, nx))
    dev = torch.device('cuda:0')
    t = lambda v: torch.tensor(np.asarray(v, dtype=float), dtype=torch.float64, device=dev)
    x0, um1 = t(X0), t(np.zeros((a.batch, kw['Bd'].shape[1])))
    target = t(0.3 * np.ones(nx))
    K = controller(kw, X0, a.eps)
    xref = torch.zeros(nx, dtype=torch.float64, device=dev, requires_grad=True)
    step, ratio, halvings = a.step, float('nan'), 0
    loss = rollout_loss(K, a.steps, x0, um1, xref, target)
    for it in range(a.iters + 1):
        print('iteration %2d: loss %.10e   step %.3g   |xref| %.4f   decrease / predicted %.4f   halvings %d'
              % (it, loss.item(), step, xref.detach().norm().item(), ratio, halvings))
        if it == a.iters:
            break
        grad, = torch.autograd.grad(loss, xref)
        _, n_weak, status, n_factor = K.prob.rollout_info()
        print('              factorizations per step %.2f   weakly active rows %d   steps not differentiated %d'
              % (n_factor.mean() / a.steps, int(n_weak.sum()), int((status != 1).sum())))
        g2 = float((grad * grad).sum().item())
        while True:                                        # Armijo: halve the step until the loss falls by a quarter of step |grad|^2
            trial = (xref.detach() - step * grad).requires_grad_(True)
            new = rollout_loss(K, a.steps, x0, um1, trial, target)
            ratio = (loss.item() - new.item()) / (step * g2) if g2 > 0 else 0.0
            if ratio >= ARMIJO or step < 1e-12:
                break
            step *= 0.5; halvings += 1
        xref, loss = trial, new
    print('tuned xref:', np.array2string(xref.detach().cpu().numpy(), precision=4))


if __name__ == '__main__':
    main()
