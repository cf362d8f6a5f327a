#!/usr/bin/env python3
"""Cost of the Riccati difference equation and its adjoint (include_ext3/mpcqp_riccati_traj.h) beside the two routes it replaces.

1024 x (n = 12, m = 3, T = 20): the dual problem of a time-varying Kalman filter (a random stable model per step and instance, 3 outputs),
device tensors throughout on torch's current stream, every call timed with a pair of HIP events: a warm-up, then the median of `reps` calls,
and `chain` calls enqueued back to back divided by their number.
  * mpcqp_dre: one k_dre<16> launch, one workgroup per instance; mpcqp_dre_adjoint with both seeds and all five gradients: one
    k_dre_adjoint<16> launch;
  * (a) the stationary route: T x batch independent algebraic Riccati solves in one mpcqp_dare call and their adjoints in one
    mpcqp_dare_adjoint call (what pympc_amd.riccati.kalman_gain per schedule entry costs; NOT the same filter);
  * (b) the same recursion as a torch loop of batched matmul / cholesky / cholesky_solve on the device, forward and backward by autograd.

    python scripts/riccati_traj_rate.py [--batch 1024] [--steps 20] [--reps 30] [--chain 20]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024); ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--reps', type=int, default=30); ap.add_argument('--chain', type=int, default=20)
    a = ap.parse_args()
    import torch
    from pympc_amd import riccati
    n, m, T, B = 12, 3, a.steps, a.batch
    dev = torch.device('cuda:0')
    stream = torch.cuda.current_stream()
    rng = np.random.default_rng(0)
    G = rng.standard_normal((T, B, n, n))
    A = G * (0.95 / np.abs(np.linalg.eigvals(G)).max(axis=-1))[..., None, None]
    Bm = rng.standard_normal((B, n, m))
    spd = lambda k: (lambda M: M @ np.swapaxes(M, -1, -2) / k + 0.5 * np.eye(k))(rng.standard_normal((B, k, k)))
    t = lambda x: torch.tensor(x, dtype=torch.float64, device=dev)
    At, Bt, Q, R, X0 = t(A), t(Bm), t(spd(n)), t(spd(m)), t(spd(n))
    X, K, status, bad = riccati.dre(At, Bt, Q, R, X0, gain_form=1)
    G_X, G_K = torch.ones_like(X), torch.ones_like(K)
    # (a): every (step, instance) pair a stationary design of its own
    Af, Bf, Qf, Rf = At.reshape(T * B, n, n), Bt.repeat(T, 1, 1), Q.repeat(T, 1, 1), R.repeat(T, 1, 1)
    Xs, Ks, sts, _, _ = riccati.dare(Af, Bf, Qf, Rf, gain_form=1)
    GXs, GKs = torch.ones_like(Xs), torch.ones_like(Ks)

    # (b): the recursion in torch
    def torch_loop(A, Bm, Q, R, X0):
        Xc, Xl, Fl = 0.5 * (X0 + X0.transpose(-1, -2)), [], []
        Xl.append(Xc)
        for k in range(T):
            BtX = Bm.transpose(-1, -2) @ Xc
            Lc = torch.linalg.cholesky(R + BtX @ Bm)
            F = torch.cholesky_solve(BtX, Lc)
            Xn = A[k].transpose(-1, -2) @ (Xc - Xc @ Bm @ F) @ A[k] + Q
            Xc = 0.5 * (Xn + Xn.transpose(-1, -2))
            Xl.append(Xc); Fl.append(F)
        return torch.stack(Xl), torch.stack(Fl)
    leaves = [p.clone().requires_grad_(True) for p in (At, Bt, Q, R, X0)]

    def torch_forward_backward():
        Xt, Ft = torch_loop(*leaves)
        return torch.autograd.grad((G_X * Xt).sum() + (G_K * Ft).sum(), leaves)

    def torch_forward():
        with torch.no_grad():
            return torch_loop(At, Bt, Q, R, X0)
    calls = dict(dre=lambda: riccati.dre(At, Bt, Q, R, X0, gain_form=1),
                 dre_adjoint=lambda: riccati.dre_adjoint(At, Bt, Q, R, X0, X, status, G_X=G_X, G_K=G_K, gain_form=1),
                 stationary_dare=lambda: riccati.dare(Af, Bf, Qf, Rf, gain_form=1),
                 stationary_dare_adjoint=lambda: riccati.dare_adjoint(Af, Bf, Qf, Rf, Xs, Ks, sts, G_X=GXs, G_K=GKs, gain_form=1),
                 torch_loop_forward=torch_forward, torch_loop_forward_backward=torch_forward_backward)
    Xt, Ft = torch_forward()
    out = dict(batch=B, shape=[n, m, T], done=int((status == 1).sum()), stationary_converged=int((sts == 1).sum()),
               torch_loop_rel_distance=float(((Xt - X).abs().max() / X.abs().max()).item()))
    for name, call in calls.items():
        call()
        stream.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.chain):
            call()
        e1.record(stream)
        e1.synchronize()
        out[name + '_ms'] = float(np.median(ms))
        out[name + '_ms_min'], out[name + '_ms_max'] = float(min(ms)), float(max(ms))
        out[name + '_chained_ms'] = e0.elapsed_time(e1) / a.chain
    out['torch_loop_backward_ms'] = out['torch_loop_forward_backward_ms'] - out['torch_loop_forward_ms']
    out['forward_over_torch_loop'] = out['torch_loop_forward_ms'] / out['dre_ms']
    out['both_over_torch_loop'] = out['torch_loop_forward_backward_ms'] / (out['dre_ms'] + out['dre_adjoint_ms'])
    out['both_over_stationary'] = (out['stationary_dare_ms'] + out['stationary_dare_adjoint_ms']) / (out['dre_ms'] + out['dre_adjoint_ms'])
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
