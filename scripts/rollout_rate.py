#!/usr/bin/env python3
"""What a taped rollout and its reverse sweep (include/mpcqp_rollout.h) cost, against what there was before them.

Random stable LTI instances (pympc_amd.fixtures.random_lti) in closed loop with their own model as the plant, on torch's current stream with
device tensors throughout (every call is stream-ordered), each figure from a pair of HIP events around the call and a synchronise, after a
warm-up of the same call.  The variants of a comparison alternate inside the repetition loop, and every repetition is printed: the spread
is part of the result.  Per (batch, shape, K):
  (a) the price of taping    rollout(K) against run(K) on the same handle, each from the same state (update + solve before it, not timed);
  (b) the reverse sweep      rollout_adjoint (x0, u_{-1}, Ad, Bd wanted) against the route without a tape: K controllers, each stepped once
                             (BatchMPCController.step), then mpcqp_adjoint_model on each in reverse with the plant's chain rule between them in torch --
                             time of both backward passes, time of both forward passes, and the device memory each route holds
                             (hipMemGetInfo before and after it is built: K handles against one handle and its tape);
  (c) the factor reuse       no_reuse = 1 against 0, with the mean n_factor / K beside it.
One JSON line per (batch, shape, K).

``--bounds``: the sweeps of (b) and (c) are asked for the six bound gradients too (include/mpcqp_adjoint_bounds.h).
``--schedule HOLD ..``: per hold, the loop under a model schedule (include_ext/mpcqp_rollout_tv.h; every entry a smooth 3 % perturbation of
the instance's Ad, Bd) in the same alternation: run(model_traj=) against rollout_tv, and the scheduled sweep ('Ad_traj', 'Bd_traj',
'Ap_traj', 'Bp_traj' in place of 'Ad', 'Bd', 'Ap', 'Bp') with its n_factor / K, beside the constant-model figures of the same repetition.
Every timed loop starts from the same model, state and solve (update_model + update + solve before it, not timed).
``--estimator`` (with ``--schedule``): the output-feedback legs in the same repetition loop -- random C with ny = 3 outputs, stationary Kalman
gains from pympc_amd.torch_layer.kalman_gain (one per instance; under a schedule one per entry) -- run(estimator=) against rollout_est and
its sweep, and per hold run(estimator=, model_traj=, L_traj=) against rollout_tv_est (include_ext2/mpcqp_rollout_tv_est.h) and its sweep, with
the plain sweep and the scheduled state-feedback sweep timed again beside them, so that the four sweeps of one repetition can be compared.

    python scripts/rollout_rate.py [--reps 5] [--eps 1e-6] [--sizes 1024:12,4,30 256:4,2,10] [--steps 20 100] [--no-route-b] [--bounds] [--schedule 1 5] [--estimator]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def controller(kws, Np, eps, stream):
    from pympc_amd import BatchMPCController
    s = lambda k: np.stack([kw[k] for kw in kws])
    K = BatchMPCController(s('Ad'), s('Bd'), Np=Np, x0=s('x0'), xref=s('xref'), uref=s('uref'), uminus1=s('uminus1'), Qx=s('Qx'), QxN=s('QxN'),
                           Qu=s('Qu'), QDu=s('QDu'), xmin=s('xmin'), xmax=s('xmax'), umin=s('umin'), umax=s('umax'), Dumin=s('Dumin'),
                           Dumax=s('Dumax'), eps_feas=1e6, eps_abs=eps, eps_rel=eps, max_iter=20000, stream=stream.cuda_stream)
    K.setup()
    return K


def estimator_leg(a, torch, t, bp, K, B, nx, nu, Ad, x0, out, gx, gu, want, want_tv, scheds, reset, timed):
    """The output-feedback legs of one (batch, shape, K): dict of lists of milliseconds, one entry per repetition; per hold under 'schedule'."""
    from pympc_amd.torch_layer import kalman_gain
    ny, dev = 3, x0.device
    rng = np.random.default_rng(5)
    Cm = t(rng.standard_normal((B, ny, nx)))
    Qn, Rn = t(0.01 * np.eye(nx)), t(0.01 * np.eye(ny))
    Lg = kalman_gain(Ad, Cm, Qn, Rn)[0]
    assert bool((Lg.status == 1).all())
    Lts = {}
    for hold, sc in scheds.items():                        # a gain per schedule entry
        nseg = sc[0].shape[0]
        Lt = kalman_gain(sc[0].reshape(nseg * B, nx, nx), Cm.repeat(nseg, 1, 1), Qn, Rn)[0]
        assert bool((Lt.status == 1).all())
        Lts[hold] = Lt.reshape(nseg, B, nx, ny).contiguous()
    oute = out + [torch.empty((K + 1, B, nx), dtype=torch.float64, device=dev), torch.empty((K, B, ny), dtype=torch.float64, device=dev)]
    seeds = dict(g_x=gx, g_u=gu, g_xhat=torch.randn((K + 1, B, nx), dtype=torch.float64, device=dev), g_y=torch.randn((K, B, ny), dtype=torch.float64, device=dev))
    est = lambda: dict(C=Cm, L=Lg, x_true=x0.clone(), v=None)
    want_e = want + ('eta', 'C', 'L', 'Ae', 'Be')
    want_x = want_tv + ('eta', 'C', 'L_traj', 'Ae_traj', 'Be_traj')
    r = dict(ny=ny, run_est_ms=[], rollout_est_ms=[], sweep_est_ms=[], sweep_plain_ms=[], tape_bytes=bp.rollout_tape_bytes(K, ny=ny))
    tv = {hold: dict(run_tv_est_ms=[], rollout_tv_est_ms=[], sweep_tv_est_ms=[], sweep_tv_ms=[], tape_bytes=bp.rollout_tv_est_tape_bytes(K, hold, ny)) for hold in scheds}
    for rep in range(a.reps + 1):                          # (repetition 0 warms every call up and is not kept)
        keep = (lambda lst, v: lst.append(v)) if rep else (lambda lst, v: None)
        reset(); e = est(); keep(r['run_est_ms'], timed(lambda: bp.mpc_run(K, out=oute, estimator=e))[0])
        reset(); e = est(); keep(r['rollout_est_ms'], timed(lambda: bp.rollout_est(K, e, out=oute))[0])
        keep(r['sweep_est_ms'], timed(lambda: bp.rollout_adjoint(want=want_e, **seeds))[0])
        info = bp.rollout_info()
        r.update(n_factor_per_step=float(info[3].mean()) / K, steps_differentiated=float((info[2] == 1).mean()))
        reset(); bp.rollout(K, out=out)
        keep(r['sweep_plain_ms'], timed(lambda: bp.rollout_adjoint(g_x=gx, g_u=gu, want=want))[0])
        for hold, sc in scheds.items():
            reset(); e = est(); keep(tv[hold]['run_tv_est_ms'], timed(lambda: bp.mpc_run_tv_est(K, sc, e, L_traj=Lts[hold], out=oute))[0])
            reset(); e = est(); keep(tv[hold]['rollout_tv_est_ms'], timed(lambda: bp.rollout_tv_est(K, sc, e, L_traj=Lts[hold], out=oute))[0])
            keep(tv[hold]['sweep_tv_est_ms'], timed(lambda: bp.rollout_adjoint(want=want_x, **seeds))[0])
            info = bp.rollout_info()
            tv[hold].update(n_factor_per_step=float(info[3].mean()) / K, steps_differentiated=float((info[2] == 1).mean()))
            reset(); bp.rollout_tv(K, sc, out=out)
            keep(tv[hold]['sweep_tv_ms'], timed(lambda: bp.rollout_adjoint(g_x=gx, g_u=gu, want=want_tv))[0])
    r['schedule'] = {str(hold): v for hold, v in tv.items()}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--eps', type=float, default=1e-6)
    ap.add_argument('--sizes', nargs='+', default=['1024:12,4,30', '256:4,2,10'])
    ap.add_argument('--steps', nargs='+', type=int, default=[20, 100])
    ap.add_argument('--no-route-b', action='store_true', help='skip the K-controller route (it builds K handles)')
    ap.add_argument('--bounds', action='store_true', help='ask the sweep for xmin, xmax, umin, umax, Dumin, Dumax as well')
    ap.add_argument('--schedule', nargs='*', type=int, default=[], help='holds of a model schedule to time the scheduled loop and sweep under')
    ap.add_argument('--estimator', action='store_true', help='time the output-feedback loops and sweeps too, under every hold of --schedule')
    a = ap.parse_args()
    if a.estimator and not a.schedule:
        ap.error('--estimator times the scheduled output-feedback loop: give --schedule HOLD ..')
    import torch
    from pympc_amd import fixtures
    dev = torch.device('cuda:0')
    stream = torch.cuda.current_stream()
    t = lambda v: torch.tensor(np.asarray(v, dtype=float), dtype=torch.float64, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def used():
        stream.synchronize()
        free, total = torch.cuda.mem_get_info()
        return total - free

    for size in a.sizes:
        B, shape = size.split(':')
        B, (nx, nu, Np) = int(B), (int(v) for v in shape.split(','))
        kws = [fixtures.random_lti(i, nx=nx, nu=nu, Np=Np, xbox=4.0, ubox=0.5, dubox=0.25) for i in range(B)]
        x0, um1 = t(np.stack([kw['x0'] for kw in kws])), t(np.zeros((B, nu)))
        Ad, Bd = t(np.stack([kw['Ad'] for kw in kws])), t(np.stack([kw['Bd'] for kw in kws]))
        for K in a.steps:
            res = dict(batch=B, shape=[nx, nu, Np], K=K, eps=a.eps, reps=a.reps, bounds=bool(a.bounds))
            m0 = used()
            C = controller(kws, Np, a.eps, stream)
            bp = C.prob
            m1 = used()
            out = [torch.empty((K + 1, B, nx), dtype=torch.float64, device=dev), torch.empty((K, B, nu), dtype=torch.float64, device=dev),
                   torch.empty((K, B), dtype=torch.int32, device=dev), torch.empty((K, B), dtype=torch.int32, device=dev)]
            gx, gu = torch.randn((K + 1, B, nx), dtype=torch.float64, device=dev), torch.randn((K, B, nu), dtype=torch.float64, device=dev)
            want = ('lam', 'uminus1', 'Ad', 'Bd', 'Ap', 'Bp') + (('xmin', 'xmax', 'umin', 'umax', 'Dumin', 'Dumax') if a.bounds else ())

            def reset():
                if a.schedule:                             # (a scheduled loop leaves its last entry under the handle)
                    bp.update_model(Ad=Ad, Bd=Bd)
                bp.update(x0, um1)
                bp.solve_async()

            scheds = {}
            for hold in a.schedule:
                nseg = (K + hold - 1) // hold
                rng = np.random.default_rng(3)
                e = np.arange(nseg).reshape(-1, 1, 1, 1)
                wave = lambda M: t(M.cpu().numpy()[None] * (1.0 + 0.03 * np.sin(0.7 * e + rng.uniform(0, 2 * np.pi, (1,) + tuple(M.shape)))))
                scheds[hold] = (wave(Ad), wave(Bd), hold)
            want_tv = tuple(k + '_traj' if k in ('Ad', 'Bd', 'Ap', 'Bp') else k for k in want)

            # (a) taping, (c) reuse: warm up, then alternate
            reset(); bp.mpc_run(K, out=out); reset(); bp.rollout(K, out=out)
            res['tape_bytes'] = bp.rollout_tape_bytes(K)
            res['handle_and_tape_bytes'] = used() - m0
            res['handle_bytes'] = m1 - m0
            bufs = bp.rollout_adjoint(g_x=gx, g_u=gu, want=want)
            bp.rollout_adjoint(g_x=gx, g_u=gu, want=want, out=bufs, no_reuse=True)
            run_ms, roll_ms, sweep_ms, noreuse_ms = [], [], [], []
            tv = {hold: dict(run_tv_ms=[], rollout_tv_ms=[], sweep_tv_ms=[]) for hold in scheds}
            for hold, sc in scheds.items():                # warm up
                reset(); bp.mpc_run(K, out=out, model_traj=sc); reset(); bp.rollout_tv(K, sc, out=out)
                bp.rollout_adjoint(g_x=gx, g_u=gu, want=want_tv)
                tv[hold]['tape_bytes'] = bp.rollout_tv_tape_bytes(K, hold)
            if scheds:
                reset(); bp.rollout(K, out=out)
            for _ in range(a.reps):
                reset(); run_ms.append(timed(lambda: bp.mpc_run(K, out=out))[0])
                reset(); roll_ms.append(timed(lambda: bp.rollout(K, out=out))[0])
                sweep_ms.append(timed(lambda: bp.rollout_adjoint(g_x=gx, g_u=gu, want=want, out=bufs))[0])
                nfac = bp.rollout_info()[3]
                noreuse_ms.append(timed(lambda: bp.rollout_adjoint(g_x=gx, g_u=gu, want=want, out=bufs, no_reuse=True))[0])
                for hold, sc in scheds.items():
                    reset(); tv[hold]['run_tv_ms'].append(timed(lambda: bp.mpc_run(K, out=out, model_traj=sc))[0])
                    reset(); tv[hold]['rollout_tv_ms'].append(timed(lambda: bp.rollout_tv(K, sc, out=out))[0])
                    tv[hold]['sweep_tv_ms'].append(timed(lambda: bp.rollout_adjoint(g_x=gx, g_u=gu, want=want_tv))[0])
                    info = bp.rollout_info()
                    tv[hold].update(n_factor_per_step=float(info[3].mean()) / K, steps_differentiated=float((info[2] == 1).mean()))
            if scheds:                                     # (the constant-model tape again, for the status read below)
                reset(); bp.rollout(K, out=out); bp.rollout_adjoint(g_x=gx, g_u=gu, want=want, out=bufs)
                res['schedule'] = {str(hold): v for hold, v in tv.items()}
            _, _, status, _ = bp.rollout_info()
            res.update(run_ms=run_ms, rollout_ms=roll_ms, sweep_ms=sweep_ms, sweep_no_reuse_ms=noreuse_ms,
                       n_factor_per_step=float(nfac.mean()) / K, steps_differentiated=float((status == 1).mean()))
            if a.estimator:
                res['estimator'] = estimator_leg(a, torch, t, bp, K, B, nx, nu, Ad, x0, out, gx, gu, want, want_tv, scheds, reset, timed)
            # (b) the route without a tape: K controllers
            if not a.no_route_b:
                m2 = used()
                Ks = [controller(kws, Np, a.eps, stream) for _ in range(K)]
                res['k_controllers_bytes'] = used() - m2
                mw = ('x0', 'uminus1', 'Ad', 'Bd')

                def forward():
                    x, u, us = x0, um1, []
                    for Kk in Ks:
                        u = Kk.step(x, u, out=torch.empty((B, nu), dtype=torch.float64, device=dev))
                        us.append(u)
                        x = torch.einsum('bij,bj->bi', Ad, x) + torch.einsum('bij,bj->bi', Bd, u)
                    return us

                def backward():
                    lam, mu = gx[K], torch.zeros((B, nu), dtype=torch.float64, device=dev)
                    dA, dB = torch.zeros_like(Ad), torch.zeros_like(Bd)
                    for k in range(K - 1, -1, -1):
                        g = gu[k] + torch.einsum('bij,bi->bj', Bd, lam) + mu
                        r = Ks[k].prob.adjoint(g_u0=g, want=mw)
                        lam = gx[k] + torch.einsum('bij,bi->bj', Ad, lam) + r['x0']
                        mu = r['uminus1']
                        dA += r['Ad']; dB += r['Bd']
                    return lam, mu, dA, dB

                forward(); backward()
                fwd_ms, bwd_ms = [], []
                for _ in range(a.reps):
                    fwd_ms.append(timed(forward)[0])
                    bwd_ms.append(timed(backward)[0])
                res.update(k_controllers_forward_ms=fwd_ms, k_controllers_backward_ms=bwd_ms)
                for Kk in Ks:
                    Kk.prob.close()
                del Ks
            print(json.dumps(res), flush=True)
            bp.close()


if __name__ == '__main__':
    main()
