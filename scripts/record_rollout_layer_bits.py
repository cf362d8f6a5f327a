"""Record the golden of tests/test_gpu_rollout_layer_bits.py with a given build of the library (on the GPU):
    python scripts/record_rollout_layer_bits.py <lib.so> [out file, default tests/golden/rollout_layer_bits.npz]
Run it at the commit whose bits are to be kept -- the parent, when a change to the Python layer above the four taped loops
(pympc_amd/solver.py, pympc_amd/torch_layer.py, pympc_amd/batch.py) claims to call the library with the same arguments and to add torch's
tensors up in the same order.

``outputs()`` is what the test compares, on case 'first' of tests/rollout_cases.py (the estimator forms: with the seeds of
tests/rollout_est_cases.py and tests/rollout_tv_est_cases.py), hold 2.  For each of mpc_rollout, mpc_rollout_est, mpc_rollout_tv and
mpc_rollout_tv_est the outputs and the gradient of every tensor input under one quadratic loss, in three configurations:
  a  own plant, disturbance, noise, everything per instance, params Ad (per instance) and Qx (unbatched), bounds umax;
  b  the plant follows the model, unbatched schedule (of Ad alone) / C / L or L_traj, params Bd unbatched: every sum formed on the device;
  c  as b with params Bd per instance, and one constant gain L where b has a gain schedule: the shared tensors' sums are formed by torch.
For each of BatchMPCController.rollout, rollout_est, rollout_tv and rollout_tv_est (own plant, disturbance, noise) rollout_adjoint for every
name that tape takes, per instance and -- the names ``batch_sum`` sums -- summed over the batch, with the sweep's counts."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

OUT = os.path.join(ROOT, 'tests', 'golden', 'rollout_layer_bits.npz')
NAME, HOLD = 'first', 2
FORMS = ('rollout', 'rollout_est', 'rollout_tv', 'rollout_tv_est')
CHAIN = ('lam', 'uminus1', 'uref', 'xref')
MODEL = ('Ad', 'Bd', 'Qx', 'QxN', 'Qu', 'QDu', 'eps_feas', 'xmin', 'xmax', 'umin', 'umax', 'Dumin', 'Dumax')      # what batch_sum sums on every tape
TV, TV_EST = ('Ad_traj', 'Bd_traj', 'Ap_traj', 'Bp_traj'), ('Ae_traj', 'Be_traj', 'L_traj')
# form -> (every name its tape takes, those of them batch_sum sums)
WANT = {
    'rollout': (CHAIN + ('Ap', 'Bp') + MODEL, MODEL),
    'rollout_est': (CHAIN + ('Ap', 'Bp', 'eta', 'C', 'L', 'v', 'Ae', 'Be') + MODEL, MODEL),
    'rollout_tv': (CHAIN + ('Ap', 'Bp') + TV + MODEL, ('Ap', 'Bp') + TV + MODEL),
    'rollout_tv_est': (CHAIN + ('Ap', 'Bp', 'eta', 'C', 'L', 'v', 'Ae', 'Be') + TV + TV_EST + MODEL, ('Ap', 'Bp', 'L', 'Ae', 'Be') + TV + TV_EST + MODEL),
}


def _case(form):
    """(the form's instance seeds, its inputs with its own plant, disturbance and noise, its schedule (Adt, Bdt, Lt) or None)."""
    import rollout_cases as rc
    import rollout_dev as rd
    import rollout_est_cases as ec
    import rollout_tv_cases as tc
    import rollout_tv_est_cases as xc
    est, tv = form.endswith('est'), '_tv' in form
    seeds = (xc.SEEDS[NAME] if tv else ec.SEEDS[NAME]) if est else rc.CASES[NAME]['seeds']
    io = rd.inputs(NAME, True, True, seeds=seeds, est=est)
    sched = None
    if tv and est:
        bi = xc.batch_instance(NAME, HOLD)
        sched = (bi['Adt'], bi['Bdt'], bi['Lt'])
    elif tv:
        sched = tc.batch_schedule(NAME, HOLD, seeds) + (None,)
    return seeds, io, sched


def _seeds(K, B, nx, nu, ny):
    rng = np.random.default_rng(41)
    return dict(g_x=rng.standard_normal((K + 1, B, nx)), g_u=rng.standard_normal((K, B, nu)), g_xhat=rng.standard_normal((K + 1, B, nx)), g_y=rng.standard_normal((K, B, ny)))


def _batch(form):
    """BatchMPCController.<form> and rollout_adjoint: name -> array."""
    import rollout_cases as rc
    import rollout_dev as rd
    est, tv = form.endswith('est'), '_tv' in form
    K = rc.CASES[NAME]['K']
    seeds, io, sched = _case(form)
    C = rd.ctrl(NAME, seeds=seeds)
    args = [K] + ([(sched[0], sched[1], HOLD)] if tv else []) + ([rd.estimator(C, io['e'], v=io['v'])] if est else [])
    tr = getattr(C, form)(*args, w=io['w'], Ap=io['Ap'], Bp=io['Bp'], **(dict(L_traj=sched[2]) if tv and est else {}))
    g = _seeds(K, C.B, C.nx, C.nu, io['e']['C'].shape[-2] if est else 1)
    if not est:
        del g['g_xhat'], g['g_y']
    res = {k: tr[k] for k in ('x', 'u', 'iter') + (('xhat', 'y') if est else ())}
    want, summed = WANT[form]
    got = C.rollout_adjoint(want=want, **g)
    res.update({k: got[k] for k in want + ('n_weak', 'status', 'n_factor')})
    tot = C.rollout_adjoint(want=summed, batch_sum=True, **g)
    res.update({'sum_' + k: tot[k] for k in summed + ('n_factor',)})
    return res


def _layer(form, conf):
    """torch_layer.mpc_<form> in configuration ``conf`` and the gradient of every tensor input: name -> array."""
    import torch
    import rollout_cases as rc
    import rollout_dev as rd
    from pympc_amd import torch_layer
    est, tv = form.endswith('est'), '_tv' in form
    K = rc.CASES[NAME]['K']
    seeds, io, sched = _case(form)
    C = rd.ctrl(NAME, seeds=seeds)
    dev = torch.device('cuda:0')
    t = lambda a: torch.tensor(np.asarray(a, dtype=float), dtype=torch.float64, device=dev, requires_grad=True)
    one = (lambda a: a) if conf == 'a' else (lambda a: a[0])            # per instance, or instance 0's for the whole batch
    ins = dict(x0=t(io['e']['x_true0'] if est else C.x0), u_prev=t(C.uminus1), xref=t(C.xref))
    if est:
        ins.update(xhat0=t(C.x0), C=t(one(io['e']['C'])))
        if tv and conf != 'c':
            ins['L_traj'] = t(sched[2] if conf == 'a' else sched[2][:, 0])
        else:
            ins['L'] = t(one(io['e']['L']))
    if tv:
        ins['Ad_traj'] = t(sched[0] if conf == 'a' else sched[0][:, 0])
        ins['Bd_traj'] = t(sched[1]) if conf == 'a' else None
    if conf == 'a':
        ins.update(w=t(io['w']), Ap=t(io['Ap']), Bp=t(io['Bp']))
        if est:
            ins['v'] = t(io['v'])
        params, bounds = dict(Ad=t(C.Ad), Qx=t(C.Qx[0])), dict(umax=t(C.umax))
    else:
        params, bounds = dict(Bd=t(C.Bd[0] if conf == 'b' else C.Bd)), None
    kw = dict(ins)
    pos = [kw.pop('x0')] + ([kw.pop('xhat0')] if est else []) + [K] + ([kw.pop('Ad_traj'), kw.pop('Bd_traj'), HOLD] if tv else []) + ([kw.pop('C')] if est else [])
    outs = getattr(torch_layer, 'mpc_' + form)(C, *pos, params=params, bounds=bounds, **kw)
    names = ('X', 'Xhat', 'Y', 'U') if est else ('X', 'U')
    g = _seeds(K, C.B, C.nx, C.nu, outs[2].shape[-1] if est else 1)
    loss = sum(0.5 * (torch.tensor(g[s], device=dev) * o * o).sum() for s, o in zip(('g_x', 'g_xhat', 'g_y', 'g_u') if est else ('g_x', 'g_u'), outs))
    leaves = {k: v for k, v in ins.items() if v is not None}
    leaves.update({'params_' + k: v for k, v in params.items()})
    leaves.update({'bounds_' + k: v for k, v in (bounds or {}).items()})
    grads = torch.autograd.grad(loss, list(leaves.values()))
    res = {n: o.detach().cpu().numpy() for n, o in zip(names, outs)}
    res.update({'d_' + k: v.cpu().numpy() for k, v in zip(leaves, grads)})
    res.update(left_Ad=C.Ad, left_Bd=C.Bd)                              # (what the controller is left with)
    return res


def outputs():
    """name -> array, every one of the eight-and-more rollouts under its own prefix."""
    res = {}
    for form in FORMS:
        res.update({'%s.batch.%s' % (form, k): v for k, v in _batch(form).items()})
        for conf in 'abc':
            res.update({'%s.%s.%s' % (form, conf, k): v for k, v in _layer(form, conf).items()})
    return {k: np.ascontiguousarray(v) for k, v in res.items()}


def save(path, arrs):
    """Some hundred small arrays: one member per array is mostly zip and npy headers, so they are kept end to end, one member per dtype (float64
    and int32 are all there is), with the names and shapes beside them."""
    names = sorted(arrs)
    assert all(arrs[k].dtype in (np.float64, np.int32) for k in names)
    flat = {d: np.concatenate([arrs[k].ravel() for k in names if arrs[k].dtype == d]) for d in (np.float64, np.int32)}
    np.savez_compressed(path, names=np.array(names), shapes=np.array([json.dumps([arrs[k].dtype.name] + list(arrs[k].shape)) for k in names]),
                        float64=flat[np.float64], int32=flat[np.int32])


def load(path):
    """name -> array of a file ``save`` wrote."""
    z = np.load(path)
    res, at = {}, dict(float64=0, int32=0)
    for k, s in zip(z['names'].tolist(), z['shapes'].tolist()):
        dtype, *shape = json.loads(s)
        n = int(np.prod(shape))
        res[k] = z[dtype][at[dtype]:at[dtype] + n].reshape(shape)
        at[dtype] += n
    return res


if __name__ == '__main__':
    from pympc_amd import _lib
    _lib.LIB_PATH = os.path.abspath(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else OUT
    arrs = outputs()
    assert all(np.isfinite(v).all() for v in arrs.values())
    os.makedirs(os.path.dirname(out), exist_ok=True)
    save(out, arrs)
    print('%s: %d arrays, %d bytes, n_factor %s' % (out, len(arrs), os.path.getsize(out), {f: arrs[f + '.batch.n_factor'].tolist() for f in FORMS}))
