"""Tuning an observer gain by gradient descent THROUGH the output-feedback loop (pympc_amd.torch_layer.mpc_rollout_est).

A batch of copies of one random (nx, nu, Np) = (12, 4, 30) controller regulates a plant it cannot see: it measures y = C x + v with three
outputs, estimates the state with xhat+ = Ad (xhat + L (y - C xhat)) + Bd u, and is updated with the estimate (the loop of
examples/closed_loop_kalman.py).  The plant differs a little from the controller's model, and every copy starts from its own state with a
wrong initial estimate.  L starts at the stationary Kalman gain (kalman_design_simple) and is then tuned with Adam against what the loop is
for: the closed-loop cost  mean_i sum_k (x_k - xref)' Qx (x_k - xref) + (u_k - uref)' Qu (u_k - uref)  of the TRUE state, under fixed noise
draws.  Forward is ONE controller rolled out with a tape (mpcqp_rollout_est), backward ONE mpcqp_rollout_adjoint_est call: one reverse
sweep on the device through controller, plant and estimator.  The gain reported at the end is the BEST iterate Adam visited, not the last:
cost1 of the closing OBSERVER_OK line is its cost, cost0 the Kalman gain's.

    python examples/differentiable_observer.py [--batch 64] [--steps 15] [--iters 30] [--lr 0.01] [--eps 1e-8]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pympc_amd import BatchMPCController, fixtures            # noqa: E402
from pympc_amd.kalman import kalman_design_simple             # noqa: E402
from pympc_amd.torch_layer import mpc_rollout_est             # noqa: E402


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
    ap.add_argument('--batch', type=int, default=64); ap.add_argument('--steps', type=int, default=15); ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--lr', type=float, default=0.01); ap.add_argument('--eps', type=float, default=1e-8)
    a = ap.parse_args()
    if a.iters < 1:
        ap.error('--iters must be at least 1 (there is nothing to compare the Kalman gain with otherwise)')
    kw = fixtures.random_lti(0)
    nx, nu = kw['Bd'].shape
    ny = 3
    rng = np.random.default_rng(0)
    Cm = rng.standard_normal((ny, nx))
    L0 = kalman_design_simple(kw['Ad'], None, Cm, None, 0.01 * np.eye(nx), 0.01 * np.eye(ny), 'filter')[0]
    X0 = kw['x0'][None] * rng.uniform(0.2, 1.0, (a.batch, 1)) + 0.05 * rng.standard_normal((a.batch, nx))      # the plant's states
    XH0 = X0 + 0.3 * rng.standard_normal((a.batch, nx))                                                           # what the controller believes
    Ap, Bp = kw['Ad'] + 0.02 * rng.standard_normal((nx, nx)), kw['Bd'] + 0.02 * rng.standard_normal((nx, nu))
    v, w = 0.02 * rng.standard_normal((a.steps, a.batch, ny)), 0.01 * rng.standard_normal((a.steps, a.batch, nx))
    dev = torch.device('cuda:0')
    t = lambda x: torch.tensor(np.asarray(x, dtype=float), dtype=torch.float64, device=dev)
    x0, xh0, um1, Ct, vt, wt, Apt, Bpt = t(X0), t(XH0), t(np.zeros((a.batch, nu))), t(Cm), t(v), t(w), t(Ap), t(Bp)
    Qx, Qu, xref, uref = t(kw['Qx']), t(kw['Qu']), t(kw['xref']), t(kw['uref'])
    K = controller(kw, XH0, a.eps)

    def cost(L):
        X, _, _, U = mpc_rollout_est(K, x0, xh0, a.steps, Ct, L, v=vt, u_prev=um1, w=wt, Ap=Apt, Bp=Bpt)
        ex, eu = X[1:] - xref, U - uref
        return (torch.einsum('kbi,ij,kbj->b', ex, Qx, ex) + torch.einsum('kbi,ij,kbj->b', eu, Qu, eu)).mean()

    L = t(L0).requires_grad_(True)
    opt = torch.optim.Adam([L], lr=a.lr)
    best, best_L, cost0, info = None, None, None, None
    for it in range(a.iters + 1):
        opt.zero_grad()
        c = cost(L)
        if cost0 is None:
            cost0 = c.item()
        if best is None or c.item() < best:
            best, best_L = c.item(), L.detach().clone()
        print('iteration %2d: closed-loop cost %.10e   |L - L_kalman| %.4f' % (it, c.item(), (L.detach() - t(L0)).norm().item()))
        if it == a.iters:
            break
        c.backward()
        info = K.prob.rollout_info()                             # (of the sweep just made)
        opt.step()
    if info is not None:
        _, n_weak, status, n_factor = info
        print('last sweep: factorizations per step %.2f   weakly active rows %d   steps not differentiated %d'
              % (n_factor.mean() / a.steps, int(n_weak.sum()), int((status != 1).sum())))
    cost1 = cost(best_L).item()
    print('best iterate: cost %.10e against %.10e at the Kalman gain; its L (first rows):\n' % (cost1, cost0), np.array2string(best_L.cpu().numpy()[:3], precision=4))
    assert cost1 < cost0, (cost0, cost1)
    print('OBSERVER_OK cost0 %.10e cost1 %.10e' % (cost0, cost1))


if __name__ == '__main__':
    main()
