#!/usr/bin/env python3
"""Median time per call of mpcqp_polish, mpcqp_adjoint (one seed) and mpcqp_gains on the three shapes whose K_pol kernels differ most:
the headline batch 1024 x (12, 4, 30) (k_polish<16>, k_adjoint<16>), 256 copies of tests/adjoint_cases.py's nb32_nu9_held (NB = 32, held
input, four columns per solve) and of nb128_nu5 (NB = 128).  Wall clock around call + wait, median of `reps` calls after a warm-up.

    python scripts/kpol_rate.py [--reps 21]            (another build: python scripts/with_lib.py <lib.so> scripts/kpol_rate.py)"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'scripts')]


def median_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=21)
    a = ap.parse_args()
    import torch
    import adjoint_cases as ac
    import adjoint_rate
    from pympc_amd import BatchMPCController
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for tag, make in (('12_4_30', lambda: adjoint_rate.batch(range(1024), 1e-3)),
                          ('nb32_nu9_held', lambda: BatchMPCController(**ac.batch_kwargs('nb32_nu9_held', [ac.CASES['nb32_nu9_held']['seeds'][0]] * 256, eps_abs=1e-9, eps_rel=1e-9, max_iter=400000))),
                          ('nb128_nu5', lambda: BatchMPCController(**ac.batch_kwargs('nb128_nu5', [ac.CASES['nb128_nu5']['seeds'][0]] * 256, eps_abs=1e-9, eps_rel=1e-9, max_iter=400000)))):
            K = make()
            if tag != '12_4_30':
                K.setup()
            bp = K.prob
            g = torch.ones((bp.batch, bp.nu), dtype=torch.float64, device='cuda:0')
            fns = dict(adjoint=lambda: (bp.adjoint(g_u0=g), bp.synchronize()), gains=lambda: (bp.gains(like=g), bp.synchronize()),
                       polish=lambda: (bp.polish(), bp.synchronize()))      # (polish last: it replaces the iterate the adjoint differentiates)
            for name, fn in fns.items():
                out['%s/%s_ms' % (tag, name)] = round(median_ms(fn, a.reps), 4)
            out[tag + '/adjoint_status_1'] = int((bp.adjoint_info()[2] == 1).sum())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
