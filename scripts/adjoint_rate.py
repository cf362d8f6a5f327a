#!/usr/bin/env python3
"""Cost of the adjoint derivatives (include/mpcqp_adjoint.h) beside solution polishing, at the headline shape and on one cart pole.

  * 1024 x (12, 4, 30) random stable LTI instances (pympc_amd.fixtures.random_lti) solved at eps 1e-3, then `reps` launches each of
    mpcqp_polish (k_polish<16>), mpcqp_adjoint with one seed (k_adjoint<16>, nseeds = 1) and mpcqp_gains (k_adjoint<16>, nseeds = nu = 4):
    wall clock per call here, kernel times from a profile of this script run on its own:
        rocprofv3 --kernel-trace --stats -- python scripts/adjoint_rate.py
    (the two k_adjoint uses are told apart with --only adjoint / --only gains, one profile each);
  * the reference's cart pole (4, 1, 20), one controller: the same three calls.

    python scripts/adjoint_rate.py [--batch 1024] [--reps 20] [--only polish|adjoint|gains] [--lib PATH]

--lib PATH loads another build of libmpcqp_hip.so (the parent commit's, to time its k_polish beside this one's kernels)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batch(idx, eps):
    from pympc_amd import BatchMPCController, fixtures
    kws = [fixtures.random_lti(int(i)) for i in idx]
    s = lambda k: np.stack([kw[k] for kw in kws])
    K = BatchMPCController(s('Ad'), s('Bd'), Np=30, x0=s('x0'), xref=s('xref'), uref=s('uref'), uminus1=s('uminus1'), Qx=s('Qx'), QxN=s('QxN'),
                           Qu=s('Qu'), QDu=s('QDu'), xmin=s('xmin'), xmax=s('xmax'), umin=s('umin'), umax=s('umax'), Dumin=s('Dumin'),
                           Dumax=s('Dumax'), eps_feas=1e6, eps_abs=eps, eps_rel=eps)
    K.setup()
    return K


def timed(fn, reps):
    fn()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t) / reps * 1e3


def calls(bp, only, have_adjoint):
    """The three calls on BatchProblem bp, each ending with a wait: name -> function."""
    import torch
    dev = torch.device('cuda:0')
    g = torch.ones((bp.batch, bp.nu), dtype=torch.float64, device=dev)
    out = {k: torch.empty(s, dtype=torch.float64, device=dev) for k, s in
           (('x0', (bp.batch, bp.nx)), ('uminus1', (bp.batch, bp.nu)), ('xref', (bp.batch, bp.nx)), ('uref', (bp.batch, bp.nu)))}

    def polish():
        bp.polish(); bp.synchronize()

    def adjoint():
        bp.adjoint(g_u0=g, out=out); bp.synchronize()

    def gains():
        bp.gains(like=g); bp.synchronize()

    fns = dict(polish=polish)
    if have_adjoint:
        fns.update(adjoint=adjoint, gains=gains)
    return {k: f for k, f in fns.items() if only in (None, k)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--only', choices=['polish', 'adjoint', 'gains'], default=None)
    ap.add_argument('--lib', default=None)
    a = ap.parse_args()
    from pympc_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    have = _lib.has_adjoint()
    out = dict(batch=a.batch, shape=[12, 4, 30], eps=1e-3, reps=a.reps, lib=a.lib or 'in-tree', has_adjoint=have)
    K = batch(range(a.batch), 1e-3)
    bp = K.prob
    for name, fn in calls(bp, a.only, have).items():
        out[name + '_ms'] = timed(fn, a.reps)
    if have and a.only is None:
        nact, nweak, status = bp.adjoint_info()
        out['status_1'] = int((status == 1).sum()); out['n_weak_instances'] = int((nweak > 0).sum())
        out['gains_over_adjoint'] = out['gains_ms'] / out['adjoint_ms']
    # one cart pole
    from pympc_amd import MPCController, fixtures
    Kc = MPCController(**fixtures.cart_pole())
    Kc.setup()
    for name, fn in calls(Kc.prob.batch_problem, a.only, have).items():
        out['cart_pole_' + name + '_us'] = timed(fn, 10 * a.reps) * 1e3
    print(json.dumps(out))


if __name__ == '__main__':
    main()
