#!/usr/bin/env python3
"""What the taped rollout with an affine term and its reverse sweep (include_ext5/mpcqp_rollout_affine.h) cost, beside the loops and sweeps
there were before them.

The method of scripts/rollout_rate.py: random stable LTI instances in closed loop with their own model as the plant, on torch's current stream
with device tensors throughout, each figure from a pair of HIP events around the call and a synchronise, after a warm-up repetition of every
call; the variants alternate inside the repetition loop, and every repetition is printed: the spread is part of the result.  Per repetition:
  plain      run(K), rollout(K) and its sweep ('lam', 'uminus1', 'Ad', 'Bd', 'Ap', 'Bp');
  scheduled  per --schedule hold: run(model_traj=), rollout_tv and its sweep (the '_traj' names);
  affine     per rows in (1, Np) and per --d-hold: run(d_traj=, d_hold=), rollout_affine and its sweep (the plain names and 'd0', 'd_traj');
             the terms are 0.05 max(1, |x0|_inf) N(0, 1), the first solve of every timed loop is made under entry 0.
With ``--older-only`` the affine legs are left out, so that the script runs against a library from before them (scripts/with_lib.py): the four
older sweeps of two libraries are compared by alternating such runs.  One JSON line.

    python scripts/rollout_affine_rate.py [--reps 7] [--eps 1e-6] [--size 1024:12,4,30] [--steps 20] [--schedule 5] [--d-hold 1 5] [--older-only]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--eps', type=float, default=1e-6)
    ap.add_argument('--size', default='1024:12,4,30')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--schedule', nargs='*', type=int, default=[5])
    ap.add_argument('--d-hold', nargs='*', type=int, default=[1, 5])
    ap.add_argument('--older-only', action='store_true', help='leave the affine legs out (a library from before them)')
    a = ap.parse_args()
    import torch
    from pympc_amd import fixtures
    from rollout_rate import controller
    dev = torch.device('cuda:0')
    stream = torch.cuda.current_stream()
    t = lambda v: torch.tensor(np.asarray(v, dtype=float), dtype=torch.float64, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    B, shape = a.size.split(':')
    B, (nx, nu, Np) = int(B), (int(v) for v in shape.split(','))
    K = a.steps
    kws = [fixtures.random_lti(i, nx=nx, nu=nu, Np=Np, xbox=4.0, ubox=0.5, dubox=0.25) for i in range(B)]
    X0 = np.stack([kw['x0'] for kw in kws])
    x0, um1 = t(X0), t(np.zeros((B, nu)))
    Ad, Bd = t(np.stack([kw['Ad'] for kw in kws])), t(np.stack([kw['Bd'] for kw in kws]))
    bp = controller(kws, Np, a.eps, stream).prob
    out = [torch.empty((K + 1, B, nx), dtype=torch.float64, device=dev), torch.empty((K, B, nu), dtype=torch.float64, device=dev),
           torch.empty((K, B), dtype=torch.int32, device=dev), torch.empty((K, B), dtype=torch.int32, device=dev)]
    gx, gu = torch.randn((K + 1, B, nx), dtype=torch.float64, device=dev), torch.randn((K, B, nu), dtype=torch.float64, device=dev)
    want = ('lam', 'uminus1', 'Ad', 'Bd', 'Ap', 'Bp')
    want_tv = tuple(k + '_traj' if k in ('Ad', 'Bd', 'Ap', 'Bp') else k for k in want)
    affine = not a.older_only

    def reset(d0=None):
        if affine:
            bp.set_affine(d0)
        bp.update_model(Ad=Ad, Bd=Bd)                      # (a scheduled loop leaves its last entry under the handle)
        bp.update(x0, um1)
        bp.solve_async()

    scheds = {}
    for hold in a.schedule:
        nseg = (K + hold - 1) // hold
        rng = np.random.default_rng(3)
        e = np.arange(nseg).reshape(-1, 1, 1, 1)
        wave = lambda M: t(M.cpu().numpy()[None] * (1.0 + 0.03 * np.sin(0.7 * e + rng.uniform(0, 2 * np.pi, (1,) + tuple(M.shape)))))
        scheds[hold] = (wave(Ad), wave(Bd), hold)
    terms = {}
    scale = 0.05 * np.maximum(1.0, np.abs(X0).max(axis=1))
    for rows in ((1, Np) if affine else ()):
        for hold in a.d_hold:
            d = scale[None, :, None, None] * np.random.default_rng(11).standard_normal(((K + hold - 1) // hold, B, rows, nx))
            terms[(rows, hold)] = t(d)

    res = dict(batch=B, shape=[nx, nu, Np], K=K, eps=a.eps, reps=a.reps, run_ms=[], rollout_ms=[], sweep_ms=[],
               schedule={str(h): dict(run_tv_ms=[], rollout_tv_ms=[], sweep_tv_ms=[]) for h in scheds},
               affine={'rows %d d_hold %d' % k: dict(run_affine_ms=[], rollout_affine_ms=[], sweep_affine_ms=[]) for k in terms})
    for rep in range(a.reps + 1):                          # (repetition 0 warms every call up and is not kept)
        keep = (lambda lst, v: lst.append(v)) if rep else (lambda lst, v: None)
        reset(); keep(res['run_ms'], timed(lambda: bp.mpc_run(K, out=out)))
        reset(); keep(res['rollout_ms'], timed(lambda: bp.rollout(K, out=out)))
        keep(res['sweep_ms'], timed(lambda: bp.rollout_adjoint(g_x=gx, g_u=gu, want=want)))
        res['n_factor_per_step'] = float(bp.rollout_info()[3].mean()) / K
        for hold, sc in scheds.items():
            r = res['schedule'][str(hold)]
            reset(); keep(r['run_tv_ms'], timed(lambda: bp.mpc_run(K, out=out, model_traj=sc)))
            reset(); keep(r['rollout_tv_ms'], timed(lambda: bp.rollout_tv(K, sc, out=out)))
            keep(r['sweep_tv_ms'], timed(lambda: bp.rollout_adjoint(g_x=gx, g_u=gu, want=want_tv)))
            r['n_factor_per_step'] = float(bp.rollout_info()[3].mean()) / K
        for (rows, hold), d in terms.items():
            r = res['affine']['rows %d d_hold %d' % (rows, hold)]
            reset(d[0]); keep(r['run_affine_ms'], timed(lambda: bp.mpc_run(K, out=out, d_traj=d, d_hold=hold)))
            reset(d[0]); keep(r['rollout_affine_ms'], timed(lambda: bp.rollout_affine(K, d_traj=d, d_hold=hold, out=out)))
            keep(r['sweep_affine_ms'], timed(lambda: bp.rollout_adjoint(g_x=gx, g_u=gu, want=want + ('d0', 'd_traj'))))
            info = bp.rollout_info()
            r.update(n_factor_per_step=float(info[3].mean()) / K, steps_differentiated=float((info[2] == 1).mean()),
                     tape_bytes=bp.rollout_affine_tape_bytes(K, rows, d_hold=hold))
    med = lambda v: float(np.median(v)) if len(v) else None
    res['medians'] = dict(sweep_ms=med(res['sweep_ms']), rollout_ms=med(res['rollout_ms']), run_ms=med(res['run_ms']),
                          **{'sweep_tv_ms hold %s' % h: med(r['sweep_tv_ms']) for h, r in res['schedule'].items()},
                          **{'sweep_affine_ms %s' % k: med(r['sweep_affine_ms']) for k, r in res['affine'].items()},
                          **{'rollout_affine_ms %s' % k: med(r['rollout_affine_ms']) for k, r in res['affine'].items()},
                          **{'run_affine_ms %s' % k: med(r['run_affine_ms']) for k, r in res['affine'].items()})
    print(json.dumps(res), flush=True)
    bp.close()


if __name__ == '__main__':
    main()
