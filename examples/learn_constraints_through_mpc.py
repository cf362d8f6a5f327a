"""Recovering an expert's actuator limits from its inputs, THROUGH the constrained controller (pympc_amd.torch_layer.mpc_step with ``bounds``).

An expert ``BatchMPCController`` runs a point mass with an input limit umax and a rate limit Dumax and answers a batch of states and previous
inputs; most answers sit on one of the two limits.  A learner has the same model and cost but LOOSE limits -- one umax and one Dumax shared
by the whole batch -- and descends

    loss = mean_i |u_learner(x_i, u_prev_i; umax, Dumax) - u_expert(x_i, u_prev_i)|^2

by plain gradient descent.  Forward puts the current limits under the learner's controller (``update_model``: new bounds on the device,
the iterate kept) and solves; backward is one ``mpcqp_adjoint_bounds`` call (include/mpcqp_adjoint_bounds.h): one active-set KKT
factorization per instance, the multipliers of the active rows summed onto the bound each sits on in a kernel behind it, the sum over the
batch on the device.  Nothing of a training step leaves the GPU but the loss that is printed.  The law is piecewise affine in the limits: a
step is halved until the loss falls by a quarter of what the gradient predicts (the rule of examples/differentiable_mpc.py).

    python examples/learn_constraints_through_mpc.py [--batch 128] [--iters 20] [--eps 1e-8] [--step 0.5]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pympc_amd import BatchMPCController, fixtures            # noqa: E402
from pympc_amd.torch_layer import mpc_step                    # noqa: E402

ARMIJO = 0.25
NAMES = ('umax', 'Dumax')


def controller(kw, X0, eps, **over):
    B = X0.shape[0]
    m = dict(kw, **over)
    st = lambda a: np.broadcast_to(np.asarray(a, dtype=float), (B,) + np.shape(a))
    K = BatchMPCController(st(m['Ad']), st(m['Bd']), Np=m['Np'], x0=X0, xref=st(m['xref']), uref=st(m['uref']), uminus1=st(m['uminus1']),
                           Qx=st(m['Qx']), QxN=st(m['QxN']), Qu=st(m['Qu']), QDu=st(m['QDu']), xmin=st(m['xmin']), xmax=st(m['xmax']),
                           umin=st(m['umin']), umax=st(m['umax']), Dumin=st(m['Dumin']), Dumax=st(m['Dumax']), eps_feas=m.get('eps_feas', 1e6),
                           eps_abs=eps, eps_rel=eps, max_iter=200000)
    K.setup(solve=False)
    return K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=128); ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--eps', type=float, default=1e-8); ap.add_argument('--step', type=float, default=0.5)
    a = ap.parse_args()
    kw = fixtures.point_mass()
    true = dict(umax=np.array([0.7]), Dumax=np.array([0.1]))          # the expert's limits
    start = dict(umax=np.array([0.9]), Dumax=np.array([0.2]))         # the learner's: loose
    rng = np.random.default_rng(0)
    X0 = np.stack([rng.uniform(-1.0, 3.0, a.batch), rng.uniform(-0.2, 0.4, a.batch)], axis=1)      # far from the reference at 7: every answer pushes
    UM1 = rng.uniform(0.0, 0.85, (a.batch, 1))                                                      # previous inputs on both sides of the input limit's reach
    dev = torch.device('cuda:0')
    t = lambda v: torch.tensor(np.asarray(v, dtype=float), dtype=torch.float64, device=dev)
    x0, um1 = t(X0), t(UM1)

    expert = controller(kw, X0, a.eps, **true)
    u_exp = mpc_step(expert, x0, um1).detach()
    assert all(s == 'solved' for s in expert.status())
    expert.gains()
    nact = expert.prob.adjoint_info()[0] - (kw['Np'] + 1) * 2
    print('expert: %d of %d states with active inequality rows (%d rows in all)' % (int((nact > 0).sum()), a.batch, int(nact.sum())))

    learner = controller(kw, X0, a.eps, **start)
    bounds = {k: t(start[k]).requires_grad_(True) for k in NAMES}     # unbatched: one limit for the batch, its gradient the device's batch sum
    dist = lambda p: {k: float(np.abs(p[k].detach().cpu().numpy() - true[k]).max()) for k in NAMES}
    loss_of = lambda p: ((mpc_step(learner, x0, um1, bounds=p) - u_exp) ** 2).sum(dim=1).mean()
    d0 = dist(bounds)
    step, ratio, halvings = a.step, float('nan'), 0
    loss = loss_of(bounds)
    for it in range(a.iters + 1):
        d = dist(bounds)
        print('iteration %2d: loss %.10e   step %.3g   umax %.6f   Dumax %.6f   decrease / predicted %.4f   halvings %d'
              % (it, loss.item(), step, bounds['umax'].item(), bounds['Dumax'].item(), ratio, halvings))
        if it == a.iters:
            break
        grads = torch.autograd.grad(loss, [bounds[k] for k in NAMES])
        g2 = float(sum((g * g).sum().item() for g in grads))
        while True:                                        # halve the step until the loss falls by a quarter of step |grad|^2
            trial = {k: (bounds[k].detach() - step * g).requires_grad_(True) for k, g in zip(NAMES, grads)}
            new = loss_of(trial)
            ratio = (loss.item() - new.item()) / (step * g2) if g2 > 0 else 0.0
            if ratio >= ARMIJO or step < 1e-12:
                break
            step *= 0.5; halvings += 1
        bounds, loss = trial, new
    d = dist(bounds)
    print('distance to the expert\'s limits: ' + '   '.join('%s %.4e -> %.4e' % (k, d0[k], d[k]) for k in NAMES))


if __name__ == '__main__':
    main()
