#!/usr/bin/env python3
"""Cost and effect of solution polishing (include/mpcqp_polish.h) at the headline shape and on one cart pole.

  * 1024 x (12, 4, 30) random stable LTI instances (pympc_amd.fixtures.random_lti) at pyMPC's tolerance eps 1e-3: a batch solve
    without and with polishing (wall clock per solve, and the polish launch alone: mpcqp_polish after an unpolished solve), and the
    u* error of both against the optimum the CPU oracle reaches at eps 1e-10 on a sample of the instances;
  * the reference's cart pole (4, 1, 20) through MPCController.update() without and with polish=True (wall clock per update).

    python scripts/polish_rate.py [--batch 1024] [--reps 20] [--sample 16]

For the polish kernel's own time, profile a run of this script on its own:  rocprofv3 --kernel-trace --stats -- python scripts/polish_rate.py
(k_polish<16> is the polish kernel; k_mpc_run the solve)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batch(idx, eps, **settings):
    from pympc_amd import BatchMPCController, fixtures
    kws = [fixtures.random_lti(int(i)) for i in idx]
    s = lambda k: np.stack([kw[k] for kw in kws])
    K = BatchMPCController(s('Ad'), s('Bd'), Np=30, x0=s('x0'), xref=s('xref'), uref=s('uref'), uminus1=s('uminus1'), Qx=s('Qx'), QxN=s('QxN'),
                           Qu=s('Qu'), QDu=s('QDu'), xmin=s('xmin'), xmax=s('xmax'), umin=s('umin'), umax=s('umax'), Dumin=s('Dumin'),
                           Dumax=s('Dumax'), eps_feas=1e6, eps_abs=eps, eps_rel=eps, **settings)
    K.setup()
    return K, kws


def timed(fn, reps):
    fn()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t) / reps * 1e3


def oracle_u0(kw, eps=1e-10):
    from pympc_amd import MPCController
    from oracle.osqp_oracle import OSQP
    kw = dict(kw, eps_abs=eps, eps_rel=eps)
    K = MPCController(**kw)
    K.prob = OSQP()
    K.solver_settings = dict(max_iter=1000000)
    K.setup()
    return K.output()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--sample', type=int, default=16)
    a = ap.parse_args()
    B = a.batch
    out = dict(batch=B, shape=[12, 4, 30], eps=1e-3)
    K0, kws = batch(range(B), 1e-3)
    K1, _ = batch(range(B), 1e-3, polish=True)
    p0, p1 = K0.prob, K1.prob
    # u* of the cold solves setup() made, against the optimum on a sample (before the timing loops: re-solving the same data warm-started
    # converges further every time)
    st = p1.polish_status()
    out['accepted'] = int((st == 1).sum()); out['rejected'] = int((st == -1).sum()); out['not_performed'] = int((st == 0).sum())
    sample = np.linspace(0, B - 1, a.sample).astype(int)
    u0, u1 = p0.u0()[sample], p1.u0()[sample]
    uo = np.stack([oracle_u0(kws[i]) for i in sample])
    scale = np.maximum(1.0, np.abs(uo).max(axis=1))
    out['u_err_rel_max'] = float((np.abs(u0 - uo).max(axis=1) / scale).max())
    out['u_err_rel_max_polished'] = float((np.abs(u1 - uo).max(axis=1) / scale).max())

    def solve(p):
        p.solve_async(); p.synchronize()
    out['solve_ms'] = timed(lambda: solve(p0), a.reps)
    out['solve_polish_ms'] = timed(lambda: solve(p1), a.reps)

    def polish_only():
        p0.polish(); p0.synchronize()
    solve(p0)
    out['polish_launch_ms'] = timed(polish_only, a.reps)      # (re-polishes the same solve: the same work every time)
    # one cart pole: MPCController.update() without / with polishing
    from pympc_amd import MPCController, fixtures
    for tag, settings in (('cart_pole_update_us', {}), ('cart_pole_update_polish_us', dict(polish=True))):
        kw = fixtures.cart_pole()
        K = MPCController(**kw)
        K.solver_settings = settings
        K.setup()
        x, u = np.array(kw['x0'], dtype=float), K.output()
        K.update(x, u)
        t = time.perf_counter()
        n = 200
        for _ in range(n):
            K.update(x, u)
        out[tag] = (time.perf_counter() - t) / n * 1e6
        out[tag.replace('_us', '_status_polish')] = int(K.res.info.status_polish)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
