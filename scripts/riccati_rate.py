#!/usr/bin/env python3
"""Cost of the batched Riccati solver and its adjoint (include/mpcqp_riccati.h) beside the host route they replace.

1024 x (12, 4) and 1024 x (20, 8) random stable LTI models (pympc_amd.fixtures.random_lti, Q = Qx, R = Qu), device tensors throughout on
torch's current stream (the calls are stream-ordered and do not wait):
  * mpcqp_dare: one k_dare<16> / k_dare<32> launch, one workgroup per model;
  * mpcqp_dare_adjoint with both seeds and all four gradients: one k_dare_adjoint<NB> launch;
each timed with a pair of HIP events around the call: a warm-up, then the median of `reps` calls, and the time of `chain` calls enqueued back
to back divided by their number (the window of one call is a fraction of a millisecond).  Beside them the host route of pympc_amd.kalman:
a loop of scipy.linalg.solve_discrete_are over the same models on this machine's CPU (it has no gradient to compare with).

    python scripts/riccati_rate.py [--batch 1024] [--reps 30] [--chain 50] [--scipy 128]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--chain', type=int, default=50)
    ap.add_argument('--scipy', type=int, default=128, help='models of the batch the scipy loop solves (its time is per model)')
    a = ap.parse_args()
    import scipy.linalg as sla
    import torch
    from pympc_amd import fixtures, riccati
    dev = torch.device('cuda:0')
    stream = torch.cuda.current_stream()
    t = lambda x: torch.tensor(x, dtype=torch.float64, device=dev)
    for nx, nu in ((12, 4), (20, 8)):
        kws = [fixtures.random_lti(i, nx=nx, nu=nu) for i in range(a.batch)]
        M = [np.stack([kw[k] for kw in kws]) for k in ('Ad', 'Bd', 'Qx', 'Qu')]
        Mt = [t(m) for m in M]
        X, K, status, iters, res = riccati.dare(*Mt)
        G_X, G_K = torch.ones_like(X), torch.ones_like(K)
        calls = dict(dare=lambda: riccati.dare(*Mt), dare_adjoint=lambda: riccati.dare_adjoint(*Mt, X, K, status, G_X=G_X, G_K=G_K))
        out = dict(batch=a.batch, shape=[nx, nu], converged=int((status == 1).sum()), steps_max=int(iters.max()), res_max=float(res.max()))
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
        n = min(a.scipy, a.batch)
        sla.solve_discrete_are(M[0][0], M[1][0], M[2][0], M[3][0])
        t0 = time.perf_counter()
        Xs = [sla.solve_discrete_are(M[0][i], M[1][i], M[2][i], M[3][i]) for i in range(n)]
        out['scipy_ms_per_model'] = (time.perf_counter() - t0) * 1e3 / n
        out['scipy_loop_ms_for_the_batch'] = out['scipy_ms_per_model'] * a.batch
        out['speedup_forward'] = out['scipy_loop_ms_for_the_batch'] / out['dare_ms']
        Xd = X[:n].cpu().numpy()
        out['max_rel_distance_from_scipy'] = float(max(np.abs(Xd[i] - Xs[i]).max() / np.abs(Xs[i]).max() for i in range(n)))
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
