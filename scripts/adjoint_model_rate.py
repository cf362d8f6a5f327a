#!/usr/bin/env python3
"""Cost of the model gradients (include/mpcqp_adjoint_model.h) beside the adjoint they follow, at the headline shape.

1024 x (12, 4, 30) random stable LTI instances (pympc_amd.fixtures.random_lti) solved at eps 1e-3 on torch's current stream; then, in the
same run on the same card, with device tensors throughout (the calls are stream-ordered and do not wait):
  * mpcqp_adjoint alone: one seed g_u0, the outputs x0, uminus1, xref, uref (one k_adjoint<16> launch);
  * mpcqp_adjoint_model with the same outputs and all seven model gradients per instance (k_adjoint<16>, k_adjoint_model);
  * the same with batch_sum (k_adjoint_model_sum behind them).
Each is timed with a pair of HIP events around the call: a warm-up, then the median of `reps` calls.

    python scripts/adjoint_model_rate.py [--batch 1024] [--reps 30]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODEL = ('Ad', 'Bd', 'Qx', 'QxN', 'Qu', 'QDu', 'eps_feas')
CHAINED = ('x0', 'uminus1', 'xref', 'uref')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=30)
    a = ap.parse_args()
    import torch
    from pympc_amd import BatchMPCController, fixtures
    dev = torch.device('cuda:0')
    stream = torch.cuda.current_stream()
    kws = [fixtures.random_lti(i) for i in range(a.batch)]
    s = lambda k: np.stack([kw[k] for kw in kws])
    K = BatchMPCController(s('Ad'), s('Bd'), Np=30, x0=s('x0'), xref=s('xref'), uref=s('uref'), uminus1=s('uminus1'), Qx=s('Qx'), QxN=s('QxN'),
                           Qu=s('Qu'), QDu=s('QDu'), xmin=s('xmin'), xmax=s('xmax'), umin=s('umin'), umax=s('umax'), Dumin=s('Dumin'),
                           Dumax=s('Dumax'), eps_feas=1e6, eps_abs=1e-3, eps_rel=1e-3, stream=stream.cuda_stream)
    K.setup()
    bp = K.prob
    g = torch.ones((bp.batch, bp.nu), dtype=torch.float64, device=dev)

    def timed(want, batch_sum):
        out = bp.adjoint(g_u0=g, want=want, batch_sum=batch_sum)       # warm-up; the buffers of the timed calls
        stream.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            bp.adjoint(g_u0=g, want=want, out=out, batch_sum=batch_sum)
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    res = dict(batch=a.batch, shape=[12, 4, 30], eps=1e-3, reps=a.reps)
    res['adjoint_ms'] = timed(CHAINED, False)
    res['adjoint_model_ms'] = timed(CHAINED + MODEL, False)
    res['adjoint_model_batch_sum_ms'] = timed(CHAINED + MODEL, True)
    res['model_outputs_ms'] = res['adjoint_model_ms'] - res['adjoint_ms']
    res['status_1'] = int((bp.adjoint_info()[2] == 1).sum())
    print(json.dumps(res))


if __name__ == '__main__':
    main()
