"""What the device tests of the taped rollouts share (tests/test_gpu_rollout.py: state feedback; tests/test_gpu_rollout_est.py: output
feedback through an estimator, ``est=True`` here): the settings and tolerances, the controller of a case, the inputs of a forward variant,
the twin that steps the same loop one launch at a time, and the forward variants themselves -- made once per process and shared.

Everything is solved at the project's parity setting eps_abs = eps_rel = 1e-9.  TOL and the central-difference bound are those of
tests/test_gpu_adjoint.py."""
import numpy as np

import rollout_cases as rc
import rollout_est_cases as ec

EPS = 1e-9
TOL = 1e-9                 # against the restatement, relative to max(1, |.|_inf)  (tests/test_gpu_adjoint.py)
FD_TOL = 1e-4              # central differences, relative to max(1, |fd|_inf)      (ibid.)
SOLVED = 1
CHAIN = ('lam', 'uminus1', 'uref', 'xref', 'Ap', 'Bp')


def case_seeds(name, est=False):
    """The seeds of a case: the state-feedback table's, or the ones the output-feedback table lists for it."""
    return ec.SEEDS[name] if est else rc.CASES[name]['seeds']


def ctrl(name, seeds=None, over=None, est=False, **settings):
    """The case's instances as a BatchMPCController, set up and solved at EPS; ``over`` replaces constructor arguments."""
    from pympc_amd import BatchMPCController
    seeds = case_seeds(name, est) if seeds is None else seeds
    args = rc.batch_kwargs(name, seeds, eps_abs=EPS, eps_rel=EPS, **dict(dict(max_iter=400000), **settings))
    args.update(over or {})
    K = BatchMPCController(**args)
    K.setup()
    return K


def estimator(K, e, v=None, x_true=None):
    from pympc_amd.kalman import BatchLinearStateEstimator
    return BatchLinearStateEstimator(K.x0, K.Ad, K.Bd, e['C'], e['L'], x_true=np.array(e['x_true0'] if x_true is None else x_true), v=v)


def inputs(name, own_plant, noisy, seeds=None, est=False):
    """One forward variant of a case: dict(Ap, Bp, w, xref_traj), None where not given; with an estimator also e = the stacked estimators
    (whose w is the disturbance) and v."""
    c = rc.CASES[name]
    seeds = case_seeds(name, est) if seeds is None else seeds
    B, K, nx, nu = len(seeds), c['K'], c['nx'], c['nu']
    rng = np.random.default_rng(17)
    dA, dB = 0.02 * rng.standard_normal((B, nx, nx)), 0.02 * rng.standard_normal((B, nx, nu))
    e = ec.batch_estimator(name, seeds) if est else None
    w = e['w'] if est else 0.01 * rng.standard_normal((K, B, nx))
    io = dict(Ap=None, Bp=None, w=w if noisy else None, xref_traj=None)
    if est:
        io.update(e=e, v=e['v'] if noisy else None)
    if own_plant:
        kws = [rc.draw(name, s)[0] for s in seeds]
        io['Ap'] = np.stack([kw['Ad'] for kw in kws]) + dA
        io['Bp'] = np.stack([kw['Bd'] for kw in kws]) + dB
    if c['tv']:
        io['xref_traj'] = np.stack([rc.xref_traj(name, s) for s in seeds], axis=1).reshape(K, B, -1)
    return io


def twin(name, io, seeds=None, est=False):
    """K calls of run(1) -- with an estimator: run(1, estimator=...) -- on one controller, with everything the handle (and the estimator)
    holds read between them: (controller, estimator or None, the K results, what was held before each)."""
    K = rc.CASES[name]['K']
    Ka = ctrl(name, seeds, est=est)
    esta = estimator(Ka, io['e']) if est else None
    seq, held = [], []
    um1, xref = np.array(Ka.uminus1), np.array(Ka.xref).reshape(Ka.B, -1)
    for k in range(K):
        x, z, y = Ka.prob.iterate_state()
        held.append(dict(x=x, z=z, y=y, status=np.array([i.status for i in Ka.prob.infos()]), um1=um1.copy(), xref=xref.copy()))
        more = {}
        if est:
            held[-1]['x_plant'] = esta.x_true.copy()
            esta.v = None if io['v'] is None else io['v'][k:k + 1]
            more['estimator'] = esta
        tr = Ka.run(1, w=None if io['w'] is None else io['w'][k:k + 1], Ap=io['Ap'], Bp=io['Bp'],
                    xref_traj=None if io['xref_traj'] is None else io['xref_traj'][k:k + 1], **more)
        if est:
            held[-1].update(x0=tr['xhat'][0].copy(), y_meas=tr['y'][0].copy())
        else:
            held[-1]['x0'] = tr['x'][0].copy()
        seq.append(tr)
        um1 = tr['u'][0].copy()
        if io['xref_traj'] is not None:
            xref = io['xref_traj'][k].copy()
    return Ka, esta, seq, held


_fwd = {False: {}, True: {}}       # (name, own_plant, noisy) -> the forward variant, state feedback and output feedback apart


def forward(name, own_plant=False, noisy=False, est=False):
    """One forward variant of a case, made once: the twin, and rollout(K) / rollout_est(K) on another controller.  The reference every test
    of the variant shares; nobody changes it."""
    key = (name, own_plant, noisy)
    if key in _fwd[est]:
        return _fwd[est][key]
    K = rc.CASES[name]['K']
    io = inputs(name, own_plant, noisy, est=est)
    Ka, esta, seq, held = twin(name, io, est=est)
    Kb = ctrl(name, est=est)
    f = dict(Ka=Ka, Kb=Kb, seq=seq, held=held, io=io, refs={})
    if est:
        estb = estimator(Kb, io['e'], v=io['v'])
        f.update(esta=esta, estb=estb, seeds=ec.SEEDS[name], tr=Kb.rollout_est(K, estb, w=io['w'], Ap=io['Ap'], Bp=io['Bp']))
    else:
        f['tr'] = Kb.rollout(K, **io)
    f['tape'] = [Kb.prob.rollout_tape(k) for k in range(K)]
    D, E, cs, _ = Kb.prob.scaling()
    f['scaling'] = (D, E, cs)
    _fwd[est][key] = f
    return f


def ref_tape(f, name, b, est=False):
    """Instance b's tape in the form of tests/rollout_ref.py (tests/rollout_est_ref.py), from the DEVICE's tape."""
    c = rc.CASES[name]
    nx, nu = c['nx'], c['nu']
    out = []
    for e in f['tape']:
        xr = e['step'][b, nx + nu:]
        out.append(dict(x=e['x'][b], z=e['z'][b], y=e['y'][b], x0=e['step'][b, :nx], um1=e['step'][b, nx:nx + nu],
                        xref=xr.reshape(-1, nx) if xr.size > nx else xr, solved=bool(e['status'][b] == SOLVED)))
        if est:
            out[-1].update(x_plant=e['x_plant'][b], y_meas=e['y_meas'][b])
    return out
