#!/usr/bin/env python3
"""What an affine term in the prediction model costs in the device loop (include_ext4/mpcqp_affine.h), in one run on 1024 x (12, 4, 30) random
stable LTI instances (pympc_amd.fixtures.random_lti) with every input resident on the device, in closed-loop solves per second:

  * no term (mpcqp_mpc_loop);
  * a constant term of Np rows (mpcqp_set_affine, then the same loop: the register-resident carry stays);
  * a schedule of terms at hold = 1 (mpcqp_mpc_loop_affine: the carry is off);
  * a schedule of references at hold = 1 (xref_traj: the carry is off too) -- the fair comparison for the third.

    python scripts/affine_rate.py [--batch 1024] [--reps 10] [--steps 20]

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
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--steps', type=int, default=20)
    a = ap.parse_args()
    B, K, nx, nu, Np = a.batch, a.steps, 12, 4, 30
    kws = [fixtures.random_lti(i) for i in range(B)]
    dev = lambda v: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64, device='cuda')
    m = {k: dev(np.stack([np.asarray(kw[k], dtype=float) for kw in kws])) for k in MODEL + ('x0', 'uminus1', 'xref')}
    m['eps_feas'] = dev(np.full((B, 1), 1e6))
    rng = np.random.default_rng(0)
    bp = BatchProblem(B, nx, nu, Np)
    bp.setup(*([m[k] for k in MODEL] + [m['eps_feas'], m['x0'], m['uminus1'], m['xref']]))
    bp.solve_async(); bp.synchronize()
    out = dict(batch=B, shape=[nx, nu, Np], steps=K, kernel=bp.kernel_name(True))
    w = dev(0.01 * rng.standard_normal((K, B, nx)))
    d = dev(0.02 * rng.standard_normal((B, Np, nx)))
    d_traj = dev(0.02 * rng.standard_normal((K, B, Np, nx)))
    xref_traj = (m['xref'][None] + dev(0.02 * rng.standard_normal((K, B, nx)))).contiguous()
    bufs = [torch.empty((K + 1, B, nx), dtype=torch.float64, device='cuda'), torch.empty((K, B, nu), dtype=torch.float64, device='cuda'),
            torch.empty((K, B), dtype=torch.int32, device='cuda'), torch.empty((K, B), dtype=torch.int32, device='cuda')]

    def loop(term, **kw):
        def run():
            bp.set_affine(term)
            bp.update(m['x0'], m['uminus1'], m['xref'])
            bp.mpc_run(K, w=w, out=bufs, **kw); bp.synchronize()
        return run
    for tag, term, kw in (('no_term', None, {}), ('constant_term', d, {}), ('term_schedule_hold1', None, dict(d_traj=d_traj)),
                          ('xref_schedule_hold1', None, dict(xref_traj=xref_traj)), ('no_term_again', None, {})):
        carried0 = bp.carry_stats()[0]
        ms = timed(loop(term, **kw), a.reps)
        out[tag + '_ms'] = ms
        out[tag + '_solves_per_s'] = B * K / (ms * 1e-3)
        out[tag + '_unsolved'] = int((bufs[2] != 1).sum().item())
        out[tag + '_carried'] = bp.carry_stats()[0] - carried0
    print(json.dumps(out))


if __name__ == '__main__':
    main()
