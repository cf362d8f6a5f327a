"""Learning a controller's model by imitation THROUGH the constrained controller (pympc_amd.torch_layer.mpc_step with ``params``).

An expert ``BatchMPCController`` has the true model (Ad, Bd) and state weight Qx and answers a batch of states, many of them with input or
rate constraints active.  A learner starts from a perturbed Ad, Bd and Qx -- ONE model shared by the whole batch -- and descends

    loss = mean_i |u_learner(x_i; Ad, Bd, Qx) - u_expert(x_i)|^2

by plain gradient descent.  Forward puts the current matrices under the learner's controller (``update_model``: re-equilibrate and
refactor on the device, keep the iterate) and solves; backward is one ``mpcqp_adjoint_model`` call (include/mpcqp_adjoint_model.h): one
active-set KKT factorization per instance, the chain rule into the matrices in a kernel behind it, the sum over the batch on the device.
Nothing of a training step leaves the GPU but the loss that is printed.  The law is piecewise smooth in the matrices: a step is halved
until the loss falls by a quarter of what the gradient predicts (the rule of examples/differentiable_mpc.py).

    python examples/learn_model_through_mpc.py [--batch 256] [--iters 30] [--eps 1e-8] [--step 2.0]
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
NAMES = ('Ad', 'Bd', 'Qx')


def controller(kw, X0, eps, **over):
    B = X0.shape[0]
    m = dict(kw, **over)
    st = lambda a: np.broadcast_to(np.asarray(a, dtype=float), (B,) + np.shape(a))
    K = BatchMPCController(st(m['Ad']), st(m['Bd']), Np=m['Np'], x0=X0, xref=st(m['xref']), uref=st(m['uref']), uminus1=st(m['uminus1']),
                           Qx=st(m['Qx']), QxN=st(m['QxN']), Qu=st(m['Qu']), QDu=st(m['QDu']), xmin=st(m['xmin']), xmax=st(m['xmax']),
                           umin=st(m['umin']), umax=st(m['umax']), Dumin=st(m['Dumin']), Dumax=st(m['Dumax']), eps_feas=m['eps_feas'],
                           eps_abs=eps, eps_rel=eps, max_iter=200000)
    K.setup(solve=False)
    return K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256); ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--eps', type=float, default=1e-8); ap.add_argument('--step', type=float, default=2.0)
    a = ap.parse_args()
    kw = fixtures.random_lti(7, nx=4, nu=2, Np=10, xbox=4.0, ubox=0.5, dubox=0.25)
    nx, nu = kw['Bd'].shape
    rng = np.random.default_rng(0)
    X0 = kw['x0'][None] * rng.uniform(0.3, 1.5, (a.batch, 1)) + 0.2 * rng.standard_normal((a.batch, nx))
    true = {k: np.asarray(kw[k], dtype=float) for k in NAMES}
    start = dict(Ad=true['Ad'] + 0.05 * rng.standard_normal((nx, nx)), Bd=true['Bd'] + 0.05 * rng.standard_normal((nx, nu)),
                 Qx=true['Qx'] @ np.diag(rng.uniform(0.8, 1.25, nx)))
    start['Qx'] = 0.5 * (start['Qx'] + start['Qx'].T)
    dev = torch.device('cuda:0')
    t = lambda v: torch.tensor(np.asarray(v, dtype=float), dtype=torch.float64, device=dev)
    x0, um1 = t(X0), t(np.zeros((a.batch, nu)))

    expert = controller(kw, X0, a.eps)
    u_exp = mpc_step(expert, x0, um1).detach()
    assert all(s == 'solved' for s in expert.status())
    expert.gains()
    nact = expert.prob.adjoint_info()[0] - (kw['Np'] + 1) * nx
    print('expert: %d of %d states with active inequality rows (%d rows in all)' % (int((nact > 0).sum()), a.batch, int(nact.sum())))

    learner = controller(kw, X0, a.eps, **start)
    params = {k: t(start[k]).requires_grad_(True) for k in NAMES}
    dist = lambda p: {k: float(np.linalg.norm(p[k].detach().cpu().numpy() - true[k])) for k in NAMES}      # (Frobenius: the norm plain descent contracts)
    loss_of = lambda p: ((mpc_step(learner, x0, um1, params=p) - u_exp) ** 2).sum(dim=1).mean()
    d0 = dist(params)
    step, ratio, halvings = a.step, float('nan'), 0
    loss = loss_of(params)
    for it in range(a.iters + 1):
        d = dist(params)
        print('iteration %2d: loss %.10e   step %.3g   |Ad - true| %.4e   |Bd - true| %.4e   |Qx - true| %.4e   decrease / predicted %.4f   halvings %d'
              % (it, loss.item(), step, d['Ad'], d['Bd'], d['Qx'], ratio, halvings))
        if it == a.iters:
            break
        grads = torch.autograd.grad(loss, [params[k] for k in NAMES])
        g2 = float(sum((g * g).sum().item() for g in grads))
        while True:                                        # halve the step until the loss falls by a quarter of step |grad|^2
            trial = {k: (params[k].detach() - step * g).requires_grad_(True) for k, g in zip(NAMES, grads)}
            new = loss_of(trial)
            ratio = (loss.item() - new.item()) / (step * g2) if g2 > 0 else 0.0
            if ratio >= ARMIJO or step < 1e-12:
                break
            step *= 0.5; halvings += 1
        params, loss = trial, new
    d = dist(params)
    print('distance to the true matrices (Frobenius): ' + '   '.join('%s %.4e -> %.4e' % (k, d0[k], d[k]) for k in NAMES))


if __name__ == '__main__':
    main()
