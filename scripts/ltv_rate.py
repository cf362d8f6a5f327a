#!/usr/bin/env python3
"""What a model change costs (include/mpcqp_model.h), in one run on 1024 x (12, 4, 30) random stable LTI instances
(pympc_amd.fixtures.random_lti) with every input resident on the device:

  * update_model(Ad, Bd): mpcqp_update_model -- pack, re-equilibration, factorization, share map; the iterate stays;
  * the route there was before: get_iterate, setup with all fourteen model fields and the step data, warm_start(x, y);
  * the device loop under a model schedule (mpcqp_mpc_loop_tv) at hold 1 and 5, and the constant-model loop (mpcqp_mpc_loop), in
    closed-loop solves per second.

    python scripts/ltv_rate.py [--batch 1024] [--reps 20] [--steps 50]

Wall clock around synchronised calls; the first call of each kind is a warm-up and not counted.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODEL = ('Ad', 'Bd', 'Qx', 'QxN', 'Qu', 'QDu', 'xmin', 'xmax', 'umin', 'umax', 'Dumin', 'Dumax', 'uref')


def timed(fn, reps):
    fn()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t) / reps * 1e3


def main():
    import torch
    from pympc_amd import fixtures
    from pympc_amd.solver import BatchProblem
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--steps', type=int, default=50)
    a = ap.parse_args()
    B, K, nx, nu, Np = a.batch, a.steps, 12, 4, 30
    kws = [fixtures.random_lti(i) for i in range(B)]
    dev = lambda v: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64, device='cuda')
    m = {k: dev(np.stack([np.asarray(kw[k], dtype=float) for kw in kws])) for k in MODEL + ('x0', 'uminus1', 'xref')}
    m['eps_feas'] = dev(np.full((B, 1), 1e6))
    rng = np.random.default_rng(0)
    # a second model per instance, 2 % away entry by entry
    Ad2 = m['Ad'] * dev(1.0 + 0.02 * rng.standard_normal((B, nx, nx)))
    Bd2 = m['Bd'] * dev(1.0 + 0.02 * rng.standard_normal((B, nx, nu)))
    bp = BatchProblem(B, nx, nu, Np)
    args = lambda Ad, Bd: [Ad, Bd] + [m[k] for k in MODEL[2:]] + [m['eps_feas'], m['x0'], m['uminus1'], m['xref']]
    bp.setup(*args(m['Ad'], m['Bd']))
    bp.solve_async(); bp.synchronize()
    out = dict(batch=B, shape=[nx, nu, Np], kernel=bp.kernel_name(True))
    flip = [0]

    def pair():
        flip[0] ^= 1
        return (Ad2, Bd2) if flip[0] else (m['Ad'], m['Bd'])

    def update_model():
        Ad, Bd = pair()
        bp.update_model(Ad=Ad, Bd=Bd); bp.synchronize()
    x, z, y = (torch.empty((B, n), dtype=torch.float64, device='cuda') for n in (bp.n, bp.m, bp.m))

    def old_route():
        from pympc_amd.solver import _ptr
        from pympc_amd import _lib
        Ad, Bd = pair()
        _lib.check(bp._L.mpcqp_get_iterate(bp._h, _ptr(x), _ptr(z), _ptr(y)), 'mpcqp_get_iterate')
        bp.setup(*args(Ad, Bd))
        bp.warm_start(x, y)
    out['update_model_ms'] = timed(update_model, a.reps)
    out['setup_route_ms'] = timed(old_route, a.reps)
    out['update_model_ms_again'] = timed(update_model, a.reps)           # (once more after the other: the order of the two does not matter)
    # the device loop: constant model, then a schedule at hold 5 and 1
    w = dev(0.01 * rng.standard_normal((K, B, nx)))
    bufs = [torch.empty((K + 1, B, nx), dtype=torch.float64, device='cuda'), torch.empty((K, B, nu), dtype=torch.float64, device='cuda'),
            torch.empty((K, B), dtype=torch.int32, device='cuda'), torch.empty((K, B), dtype=torch.int32, device='cuda')]
    e = torch.arange(K, device='cuda', dtype=torch.float64).reshape(K, 1, 1, 1)
    Adt = (m['Ad'][None] * (1.0 + 0.03 * torch.sin(0.7 * e + dev(rng.uniform(0, 6.28, (B, nx, nx)))[None]))).contiguous()
    Bdt = (m['Bd'][None] * (1.0 + 0.03 * torch.sin(0.7 * e + dev(rng.uniform(0, 6.28, (B, nx, nu)))[None]))).contiguous()

    def loop(hold):
        def run():
            bp.update(m['x0'], m['uminus1'])
            bp.mpc_run(K, w=w, out=bufs, model_traj=None if not hold else (Adt, Bdt, hold)); bp.synchronize()
        return run
    bp.update_model(Ad=m['Ad'], Bd=m['Bd']); bp.solve_async(); bp.synchronize()
    for tag, hold in (('loop_const', 0), ('loop_tv_hold5', 5), ('loop_tv_hold1', 1)):
        ms = timed(loop(hold), max(1, a.reps // 5))
        out[tag + '_ms'] = ms
        out[tag + '_solves_per_s'] = B * K / (ms * 1e-3)
        out[tag + '_unsolved'] = int((bufs[2] != 1).sum().item())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
