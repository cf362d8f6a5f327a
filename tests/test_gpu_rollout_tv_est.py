"""The output-feedback loop under a model (and gain) schedule, its tape and its reverse sweep on the device
(include_ext2/mpcqp_rollout_tv_est.h, pympc_amd/csrc/mpcqp_rollout.h: k_rollout_adjoint_tv_est) on the loops of
tests/rollout_tv_est_cases.py: the taped rollout against run(estimator=, model_traj=, L_traj=), bit for bit; tape, slots and gains against a
twin stepped on the host; the sweep against the numpy restatement tests/rollout_tv_est_ref.py evaluated on the device's own tape, slots
and gains; determinism; the reductions to the unscheduled gain and to rollout_est; central differences of run() itself; the refusals and
the kinds of tape; torch; the example.

Everything is solved at the project's parity setting eps_abs = eps_rel = 1e-9.  TOL and FD_TOL are those of tests/rollout_dev.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bounds_ref
import rollout_cases as rc
import rollout_ref as rr
import rollout_dev as rd
import rollout_tv_est_cases as xc
import rollout_tv_est_ref as xr
from rollout_dev import TOL, FD_TOL, SOLVED
from util import rel1_any as _rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WEIGHTS = xr.WEIGHT_NAMES
BOUNDS = bounds_ref.NAMES
BASE = ('lam', 'uminus1', 'uref', 'xref', 'eta', 'C', 'v')   # what neither schedule splits
TRAJ = ('Ad_traj', 'Bd_traj', 'Ap_traj', 'Bp_traj', 'Ae_traj', 'Be_traj', 'L_traj')
SUMS = ('Ad', 'Bd', 'Ap', 'Bp', 'Ae', 'Be', 'L')
ALL = BASE + TRAJ + SUMS + WEIGHTS + BOUNDS
PER_STEP = ('lam', 'eta', 'xref', 'v')
NAMES = xc.NAMES
SAME_LOOP = dict(scaling=0, warm_start=0, adaptive_rho=0)      # (tests/test_gpu_rollout_tv.py, section 5, says why)


def _ctrl(name, **kw):
    return rd.ctrl(name, seeds=xc.SEEDS[name], **kw)


_ins = {}


def _inputs(name, hold, own_plant, noisy):
    """One forward variant: dict(Ap, Bp, w, v, e = the stacked estimators with the constant gain, Adt, Bdt, Lt)."""
    key = (name, hold, own_plant, noisy)
    if key not in _ins:
        io = rd.inputs(name, own_plant, noisy, seeds=xc.SEEDS[name], est=True)
        bi = xc.batch_instance(name, hold)
        assert io['xref_traj'] is None and np.array_equal(bi['C'], io['e']['C']) and np.array_equal(bi['w'], io['e']['w'])
        _ins[key] = dict(Ap=io['Ap'], Bp=io['Bp'], w=io['w'], v=io['v'], e=io['e'], Adt=bi['Adt'], Bdt=bi['Bdt'], Lt=bi['Lt'])
    return _ins[key]


def _plant(io):
    return dict(w=io['w'], Ap=io['Ap'], Bp=io['Bp'])


_fwd = {}


def _forward(name, hold, own_plant=False, noisy=False):
    """One forward variant of a case, made once: rollout_tv_est(K) on one controller, its tape, slots and gains.  Nobody changes it."""
    key = (name, hold, own_plant, noisy)
    if key not in _fwd:
        K = rc.CASES[name]['K']
        io = _inputs(name, hold, own_plant, noisy)
        Kb = _ctrl(name)
        est = rd.estimator(Kb, io['e'], v=io['v'])
        res = Kb.rollout_tv_est(K, (io['Adt'], io['Bdt'], hold), est, L_traj=io['Lt'], **_plant(io))
        nseg = -(-K // hold)
        _fwd[key] = dict(Kb=Kb, est=est, tr=res, io=io, nseg=nseg, tape=[Kb.prob.rollout_tape(k) for k in range(K)],
                         slots=[Kb.prob.rollout_tv_slot(s) for s in range(nseg + 1)], gains=np.stack([Kb.prob.rollout_tv_est_gain(e) for e in range(nseg)]), bmaps={})
    return _fwd[key]


def _slot_parts(name, blob):
    nx, nu = rc.CASES[name]['nx'], rc.CASES[name]['nu']
    B = blob.shape[0]
    return blob[:, :nx * nx].reshape(B, nx, nx), blob[:, nx * nx:nx * nx + nx * nu].reshape(B, nx, nu), blob[:, nx * nx + nx * nu:]


def _seeds(name, B=None):
    c = rc.CASES[name]
    B = len(xc.SEEDS[name]) if B is None else B
    K, nx, nu, ny = c['K'], c['nx'], c['nu'], 2 if c['nx'] < 12 else 3
    rng = np.random.default_rng(41)
    return dict(g_x=rng.standard_normal((K + 1, B, nx)), g_xhat=rng.standard_normal((K + 1, B, nx)), g_u=rng.standard_normal((K, B, nu)), g_y=rng.standard_normal((K, B, ny)))


def _reference(f, name, hold, b, g):
    """The restatement's sweep of instance b on the device's tape, slots and gains."""
    kw, attrs = rc.draw(name, xc.SEEDS[name][b])
    tape = rd.ref_tape(f, name, b, est=True)
    if b not in f['bmaps']:
        f['bmaps'][b] = bounds_ref.bound_maps(rr.entry_kwargs(kw, tape[0]), attrs)
    slots = []
    for s in f['slots']:
        Ad, Bd, _ = _slot_parts(name, s['model'])
        slots.append(dict(Ad=Ad[b], Bd=Bd[b], D=s['D'][b], E=s['E'][b], c=s['c'][b]))
    io = f['io']
    return xr.sweep(kw, attrs, tape, slots, hold, io['e']['C'][b], f['gains'][:, b], g['g_x'][:, b], g['g_xhat'][:, b], g['g_u'][:, b], g['g_y'][:, b],
                    Ap=None if io['Ap'] is None else io['Ap'][b], Bp=None if io['Bp'] is None else io['Bp'][b], bmaps=f['bmaps'][b])


def _pairs(got, ref, b):
    """(name, the device's value, the restatement's) of every output of instance b, for a schedule that gave both matrices."""
    out = [(k, got[k][:, b] if k in PER_STEP else got[k][b], ref[k]) for k in BASE + WEIGHTS + BOUNDS]
    out += [('Ad_traj', got['Ad_traj'][:, b], ref['Ad_slots'][1:]), ('Bd_traj', got['Bd_traj'][:, b], ref['Bd_slots'][1:]),
            ('Ad', got['Ad'][b], ref['Ad_slots'][0]), ('Bd', got['Bd'][b], ref['Bd_slots'][0])]
    for k, r in (('Ap', 'Ap_entries'), ('Bp', 'Bp_entries'), ('Ae', 'Ae_entries'), ('Be', 'Be_entries'), ('L', 'L_entries')):
        out += [(k + '_traj', got[k + '_traj'][:, b], ref[r]), (k, got[k][b], ref[r].sum(axis=0))]
    return out


def _books(K, est):
    return (K.Ad, K.Bd, K.x0_rh, K.uminus1_rh, est.x, est.x_true, est.L, est.A, est.Bm, np.array(K.solve_count))


def _same_state(Ka, Kb):
    for va, vb in zip(Ka.prob.iterate_state(), Kb.prob.iterate_state()):
        assert np.array_equal(va, vb)
    (xa, ya, ia), (xb, yb, ib) = Ka.prob.solution(), Kb.prob.solution()
    assert np.array_equal(xa, xb) and np.array_equal(ya, yb) and [bytes(i) for i in ia] == [bytes(i) for i in ib]


# ---- 1. forward against the loop -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hold', ('1', '2', 'K+1'))
@pytest.mark.parametrize('name', NAMES)
def test_rollout_tv_est_is_run_with_estimator_and_schedule(name, hold):
    K = rc.CASES[name]['K']
    hold = K + 1 if hold == 'K+1' else int(hold)
    for own_plant, noisy in ((False, False), (True, True)):
        io = _inputs(name, hold, own_plant, noisy)
        sched = (io['Adt'], io['Bdt'], hold)
        if hold <= 2:
            f = _forward(name, hold, own_plant, noisy)
            Kb, estb, got = f['Kb'], f['est'], f['tr']
        else:                                              # one entry for the whole loop
            assert io['Adt'].shape[0] == 1
            Kb = _ctrl(name)
            estb = rd.estimator(Kb, io['e'], v=io['v'])
            got = Kb.rollout_tv_est(K, sched, estb, L_traj=io['Lt'], **_plant(io))
        Kd = _ctrl(name)
        estd = rd.estimator(Kd, io['e'], v=io['v'])
        want = Kd.run(K, estimator=estd, model_traj=sched, L_traj=io['Lt'], **_plant(io))
        for k in ('x', 'xhat', 'y', 'u', 'status', 'iter'):
            assert np.array_equal(got[k], want[k]), (name, hold, k)
        assert np.all(got['status'] == SOLVED)
        _same_state(Kb, Kd)
        for a, b in zip(_books(Kb, estb), _books(Kd, estd)):
            assert np.array_equal(a, b), (name, hold)
        last = (K - 1) // hold
        assert np.array_equal(Kb.Ad, io['Adt'][last]) and np.array_equal(Kb.Bd, io['Bdt'][last]) and np.array_equal(estb.L, io['Lt'][last])
        assert np.array_equal(estb.x, got['xhat'][-1]) and np.array_equal(estb.x_true, got['x'][-1]) and np.array_equal(Kb.x0_rh, got['xhat'][-1])
        for k in range(K):                                 # the estimator stepped under the entry in force with its gain
            e = k // hold
            A, Bm, L = io['Adt'][e], io['Bdt'][e], io['Lt'][e]
            inn = got['y'][k] - np.einsum('bij,bj->bi', io['e']['C'], got['xhat'][k])
            xh = np.einsum('bij,bj->bi', A, got['xhat'][k] + np.einsum('bij,bj->bi', L, inn)) + np.einsum('bij,bj->bi', Bm, got['u'][k])
            assert np.allclose(xh, got['xhat'][k + 1], rtol=1e-12, atol=1e-13), (name, hold, k)
    # without a gain schedule: the estimator's own gain throughout, and it keeps it
    io = _inputs(name, hold, False, True)
    sched = (io['Adt'], io['Bdt'], hold)
    Ka, Kc = _ctrl(name), _ctrl(name)
    esta, estc = rd.estimator(Ka, io['e'], v=io['v']), rd.estimator(Kc, io['e'], v=io['v'])
    a = Ka.rollout_tv_est(K, sched, esta, **_plant(io))
    c = Kc.run(K, estimator=estc, model_traj=sched, **_plant(io))
    for k in ('x', 'xhat', 'y', 'u', 'status', 'iter'):
        assert np.array_equal(a[k], c[k]), (name, hold, k)
    _same_state(Ka, Kc)
    for u, v in zip(_books(Ka, esta), _books(Kc, estc)):
        assert np.array_equal(u, v), (name, hold)
    assert np.array_equal(esta.L, io['e']['L'])
    assert np.array_equal(Ka.prob.rollout_tv_est_gain(0), io['e']['L']) and np.array_equal(Ka.prob.rollout_tv_est_gain(-(-K // hold) - 1), io['e']['L'])


# ---- 2. tape, slots and gains against the host ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hold', xc.HOLDS)
@pytest.mark.parametrize('name', NAMES)
def test_tape_slots_and_gains_are_what_a_twin_on_the_host_held(name, hold):
    nx, nu, K = rc.CASES[name]['nx'], rc.CASES[name]['nu'], rc.CASES[name]['K']
    for own_plant, noisy in ((False, False), (True, True)):
        f = _forward(name, hold, own_plant, noisy)
        io = f['io']
        Ka = _ctrl(name)
        esta = rd.estimator(Ka, io['e'])
        models = [dict(zip(('D', 'E', 'c'), Ka.prob.scaling()[:3]), Ad=Ka.Ad.copy(), Bd=Ka.Bd.copy())]
        um1, xref = np.array(Ka.uminus1), np.array(Ka.xref).reshape(Ka.B, -1)
        for k in range(K):
            x, z, y = Ka.prob.iterate_state()
            status = np.array([i.status for i in Ka.prob.infos()])
            x_plant = esta.x_true.copy()
            e = k // hold
            if k % hold == 0:
                Ka.update_model(Ad=io['Adt'][e], Bd=io['Bdt'][e], solve=False)
                models.append(dict(zip(('D', 'E', 'c'), Ka.prob.scaling()[:3]), Ad=io['Adt'][e], Bd=io['Bdt'][e]))
            esta.L = io['Lt'][e]
            esta.v = None if io['v'] is None else io['v'][k:k + 1]
            t = Ka.run(1, w=None if io['w'] is None else io['w'][k:k + 1], Ap=io['Ap'], Bp=io['Bp'], estimator=esta)
            for v in ('x', 'xhat'):
                assert np.array_equal(f['tr'][v][k], t[v][0]) and np.array_equal(f['tr'][v][k + 1], t[v][1]), (name, hold, k, v)
            for v in ('y', 'u', 'status', 'iter'):
                assert np.array_equal(f['tr'][v][k], t[v][0]), (name, hold, k, v)
            en = f['tape'][k]
            for v, h in (('x', x), ('z', z), ('y', y), ('status', status), ('x_plant', x_plant), ('y_meas', t['y'][0])):
                assert np.array_equal(en[v], h), (name, hold, k, v)
            assert np.array_equal(en['step'][:, :nx], t['xhat'][0]) and np.array_equal(en['step'][:, nx:nx + nu], um1), (name, hold, k)
            assert np.array_equal(en['step'][:, nx + nu:], xref), (name, hold, k)
            um1 = t['u'][0].copy()
        _same_state(Ka, f['Kb'])
        assert len(f['slots']) == len(models) == f['nseg'] + 1
        rest0 = _slot_parts(name, f['slots'][0]['model'])[2]
        for s, (slot, m) in enumerate(zip(f['slots'], models)):
            Ad, Bd, rest = _slot_parts(name, slot['model'])
            assert np.array_equal(Ad, m['Ad']) and np.array_equal(Bd, m['Bd']) and np.array_equal(rest, rest0), (name, hold, s)
            for v in ('D', 'E', 'c'):
                assert np.array_equal(slot[v], m[v]), (name, hold, s, v)
        assert np.array_equal(f['gains'], io['Lt'][:f['nseg']])
    bp = f['Kb'].prob
    ny = io['e']['C'].shape[1]
    assert bp.rollout_tv_est_tape_bytes(K, hold, ny) > max(bp.rollout_tv_tape_bytes(K, hold), bp.rollout_tape_bytes(K, ny=ny))
    with pytest.raises(RuntimeError, match=r'\(-1\)'):
        bp.rollout_tv_est_gain(f['nseg'])
    with pytest.raises(RuntimeError, match=r'\(-1\)'):
        bp.rollout_tv_est_gain(-1)


# ---- 3. the reverse sweep against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('own_plant', (False, True), ids=('plant_follows', 'plant_given'))
@pytest.mark.parametrize('hold', xc.HOLDS)
@pytest.mark.parametrize('name', NAMES)
def test_the_sweep_is_the_restatement(name, hold, own_plant):
    f = _forward(name, hold, own_plant, own_plant)
    Kb, K, nseg = f['Kb'], rc.CASES[name]['K'], f['nseg']
    g = _seeds(name)
    got = Kb.rollout_adjoint(want=ALL, **g)
    nact, nweak, status, nfac = Kb.prob.rollout_info()
    assert np.all(status == 1) and np.all(nweak == 0), (name, status, nweak)
    ny = g['g_y'].shape[-1]
    assert got['Ae_traj'].shape == (nseg, Kb.B, Kb.nx, Kb.nx) and got['Be_traj'].shape == (nseg, Kb.B, Kb.nx, Kb.nu) and got['L_traj'].shape == (nseg, Kb.B, Kb.nx, ny)
    errs = {}
    for b in range(Kb.B):
        ref = _reference(f, name, hold, b, g)
        assert np.array_equal(nact[:, b], ref['n_active']) and np.array_equal(nweak[:, b], ref['n_weak']), (name, b, nact[:, b], ref['n_active'])
        assert nfac[b] == ref['n_factor'], (name, hold, b, nfac[b], ref['n_factor'])
        for k, v, r in _pairs(got, ref, b):
            errs[k] = max(errs.get(k, 0.0), _rel(v, r))
        if hold == 1:                                      # the last entry's only solve is the one for x_K, which is on no tape; estimator and plant stepped under it
            assert np.all(got['Ad_traj'][-1, b] == 0.0) and np.all(got['Bd_traj'][-1, b] == 0.0)
            assert np.abs(got['Ae_traj'][-1, b]).max() > 0.0 and np.abs(got['L_traj'][-1, b]).max() > 0.0
    worst = max(errs.values())
    print('ROLLOUT_TV_EST_ERR %s hold %d plant %s: max %.3e  %s' % (name, hold, 'given' if own_plant else 'follows', worst, ' '.join('%s=%.1e' % kv for kv in errs.items())))
    assert worst <= TOL, (name, hold, errs)
    assert min(np.abs(got[k]).max() for k in ('Ae_traj', 'Be_traj', 'L_traj', 'C', 'v', 'eta')) > 1e-3      # (paths that are there)


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ('first', 'held'))
def test_two_sweeps_reuse_batch_sum_and_single_names(name):
    f = _forward(name, 2)
    Kb, K = f['Kb'], rc.CASES[name]['K']
    g = _seeds(name)
    a = Kb.rollout_adjoint(want=ALL, **g)
    b = Kb.rollout_adjoint(want=ALL, **g)
    c = Kb.rollout_adjoint(want=ALL, no_reuse=True, **g)
    for k in ALL + ('n_weak', 'status'):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), (name, k)
    assert np.array_equal(a['n_factor'], b['n_factor']) and np.all(c['n_factor'] == K) and np.all(a['n_factor'] <= K)
    for want in (('L_traj',), ('Ae_traj', 'Bd_traj'), ('Be',), ('C',), ('eta', 'Ad_traj')):      # asked for on their own: the same bits
        d = Kb.rollout_adjoint(want=want, **g)
        for k in want:
            assert np.array_equal(d[k], a[k]) and np.abs(d[k]).max() > 0.0, (name, want, k)
    only_y = Kb.rollout_adjoint(g_y=g['g_y'], want=('L_traj', 'v'))      # any one of the four seeds is enough
    assert np.abs(only_y['L_traj']).max() > 0.0 and not np.array_equal(only_y['L_traj'], a['L_traj'])
    s1 = Kb.rollout_adjoint(want=TRAJ + SUMS + WEIGHTS + BOUNDS, batch_sum=True, **g)
    s2 = Kb.rollout_adjoint(want=TRAJ + SUMS + WEIGHTS + BOUNDS, batch_sum=True, **g)
    for k in TRAJ:
        assert s1[k].shape[1] == 1 and np.array_equal(s1[k], s2[k]), k
        assert _rel(s1[k][:, 0], a[k].sum(axis=1)) <= 1e-13, k
    for k in SUMS + WEIGHTS + BOUNDS:
        assert s1[k].shape[0] == 1 and np.array_equal(s1[k], s2[k]), k
        assert _rel(s1[k][0], a[k].sum(axis=0)) <= 1e-13, k


# ---- 5. the reductions -----------------------------------------------------------------------------------------------------------------------
def test_a_gain_schedule_of_equal_entries_is_the_unscheduled_gain():
    name, hold = xc.FIRST, 2
    K = rc.CASES[name]['K']
    io = _inputs(name, hold, False, True)
    sched = (io['Adt'], io['Bdt'], hold)
    Lt = np.ascontiguousarray(np.repeat(io['e']['L'][None], -(-K // hold), axis=0))
    Ka, Kb = _ctrl(name), _ctrl(name)
    ta = Ka.rollout_tv_est(K, sched, rd.estimator(Ka, io['e'], v=io['v']), **_plant(io))
    tb = Kb.rollout_tv_est(K, sched, rd.estimator(Kb, io['e'], v=io['v']), L_traj=Lt, **_plant(io))
    for k in ('x', 'xhat', 'y', 'u', 'status', 'iter'):
        assert np.array_equal(ta[k], tb[k]), k
    g = _seeds(name)
    a, b = Ka.rollout_adjoint(want=ALL, **g), Kb.rollout_adjoint(want=ALL, **g)
    for k in ALL + ('n_factor', 'status'):
        assert np.array_equal(a[k], b[k]), k
    assert _rel(b['L_traj'].sum(axis=0), b['L']) <= 1e-13 and np.abs(b['L']).max() > 1e-3


@pytest.mark.parametrize('hold', xc.HOLDS)
def test_a_constant_schedule_is_rollout_est(hold):
    """Under SAME_LOOP a schedule whose every entry is the controller's own model, with the estimator's own gain, gives the forward bits of
    rollout_est, and the per-slot and per-entry sums meet its gradients within 1e-13."""
    name = xc.FIRST
    K = rc.CASES[name]['K']
    nseg = -(-K // hold)
    io = _inputs(name, hold, False, True)
    Ku, Kc = _ctrl(name, **SAME_LOOP), _ctrl(name, **SAME_LOOP)
    tu = Ku.rollout_est(K, rd.estimator(Ku, io['e'], v=io['v']), **_plant(io))
    sched = (np.repeat(Kc.Ad[None], nseg, axis=0), np.repeat(Kc.Bd[None], nseg, axis=0), hold)
    ts = Kc.rollout_tv_est(K, sched, rd.estimator(Kc, io['e'], v=io['v']), **_plant(io))
    for k in ('x', 'xhat', 'y', 'u', 'status', 'iter'):
        assert np.array_equal(ts[k], tu[k]), k
    g = _seeds(name)
    ref = Ku.rollout_adjoint(want=('lam', 'uminus1', 'uref', 'xref', 'Ap', 'Bp', 'eta', 'C', 'L', 'v', 'Ae', 'Be', 'Ad', 'Bd') + WEIGHTS + BOUNDS, **g)
    got = Kc.rollout_adjoint(want=ALL, **g)
    assert np.all(ref['status'] == 1) and np.all(got['status'] == 1)
    errs = dict(Ad=_rel(got['Ad'] + got['Ad_traj'].sum(axis=0), ref['Ad']), Bd=_rel(got['Bd'] + got['Bd_traj'].sum(axis=0), ref['Bd']))
    for k in ('Ap', 'Bp', 'Ae', 'Be', 'L'):
        errs[k] = _rel(got[k + '_traj'].sum(axis=0), ref[k])
        assert _rel(got[k + '_traj'].sum(axis=0), got[k]) <= 1e-13, k
    errs.update({k: _rel(got[k], ref[k]) for k in BASE + WEIGHTS + BOUNDS})
    print('ROLLOUT_TV_EST_CONST hold %d: %s' % (hold, ' '.join('%s=%.1e' % kv for kv in errs.items())))
    assert max(errs.values()) <= 1e-13, errs


# ---- 6. end to end: central differences of run(estimator=, model_traj=, L_traj=) itself ---------------------------------------------------
def test_the_sweep_against_central_differences_of_the_device_loop():
    """L = sum <Gx, x> + <Gxh, xhat> + <Gu, u> + <Gy, y> of run(K, estimator=, model_traj=, L_traj=) on fresh controllers, in a direction of
    xhat0, one of the whole Ad schedule (the plant follows it: solve, estimator and plant paths) and one of the whole gain schedule.  h as in
    tests/test_gpu_rollout_tv.py."""
    name, hold = xc.FIRST, 2
    K, B = rc.CASES[name]['K'], len(xc.SEEDS[name])
    g = _seeds(name)
    f = _forward(name, hold, False, True)
    io = f['io']
    got = f['Kb'].rollout_adjoint(want=('eta', 'Ad_traj', 'Ap_traj', 'Ae_traj', 'L_traj'), **g)
    assert np.all(got['status'] == 1) and np.all(got['n_weak'] == 0)
    base = rc.batch_kwargs(name, xc.SEEDS[name])
    rng = np.random.default_rng(43)
    h = 1e-4

    def loss(xh0, At, Lt):
        Kf = _ctrl(name, over=dict(x0=xh0))
        t = Kf.run(K, estimator=rd.estimator(Kf, io['e'], v=io['v']), model_traj=(At, io['Bdt'], hold), L_traj=Lt, **_plant(io))
        return sum((g[s] * t[k]).sum(axis=(0, 2)) for s, k in (('g_x', 'x'), ('g_xhat', 'xhat'), ('g_u', 'u'), ('g_y', 'y')))      # per instance: they are independent

    def unit(shape, axis_b):
        d = rng.standard_normal(shape)
        n = np.sqrt((np.moveaxis(d, axis_b, 0).reshape(B, -1) ** 2).sum(axis=1))
        return d / n.reshape([B if i == axis_b else 1 for i in range(d.ndim)])

    x0, At, Lt = base['x0'], io['Adt'], io['Lt']
    d = unit(x0.shape, 0)
    checks = [('xhat0', (got['eta'][0] * d).sum(axis=1), (loss(x0 + h * d, At, Lt) - loss(x0 - h * d, At, Lt)) / (2 * h))]
    d = unit(At.shape, 1)
    checks.append(('Ad_traj', ((got['Ad_traj'] + got['Ap_traj'] + got['Ae_traj']) * d).sum(axis=(0, 2, 3)), (loss(x0, At + h * d, Lt) - loss(x0, At - h * d, Lt)) / (2 * h)))
    d = unit(Lt.shape, 1)
    checks.append(('L_traj', (got['L_traj'] * d).sum(axis=(0, 2, 3)), (loss(x0, At, Lt + h * d) - loss(x0, At, Lt - h * d)) / (2 * h)))
    for field, an, fd in checks:
        err = np.abs(an - fd).max()
        print('ROLLOUT_TV_EST_FD d/d%s: |grad.d - FD|_inf = %.3e, |FD|_inf = %.3e' % (field, err, np.abs(fd).max()))
        assert err <= FD_TOL * max(1.0, np.abs(fd).max()), (field, err, an, fd)
        assert np.abs(fd).max() > 1e-2


# ---- 7. the refusals and the kinds of tape ---------------------------------------------------------------------------------------------------
def test_refusals_and_the_kinds_of_tape():
    from pympc_amd import _lib
    name, hold, seeds = xc.FIRST, 2, (0, 3)
    c = rc.CASES[name]
    K, nx, nu = c['K'], c['nx'], c['nu']
    full = _inputs(name, hold, False, True)
    pick = [xc.SEEDS[name].index(s) for s in seeds]
    Adt, Bdt, Lt = (np.ascontiguousarray(full[k][:, pick]) for k in ('Adt', 'Bdt', 'Lt'))
    e = {k: np.ascontiguousarray(v[:, pick] if k in ('v', 'w') else v[pick]) for k, v in full['e'].items()}
    Kt = rd.ctrl(name, seeds=seeds)
    bp = Kt.prob
    L, h = bp._L, bp._h
    g = _seeds(name, B=2)
    ny = g['g_y'].shape[-1]
    sched = (Adt, Bdt, hold)
    x_true = e['x_true0'].copy()
    out = [np.empty((K + 1, 2, nx)), np.empty((K, 2, nu)), np.empty((K, 2), dtype=np.int32), np.empty((K, 2), dtype=np.int32), np.empty((K + 1, 2, nx)), np.empty((K, 2, ny))]

    def loop(**change):
        lo = _lib.Loop()
        lo.ny, lo.C, lo.Lgain, lo.x_true = ny, e['C'].ctypes.data, e['L'].ctypes.data, x_true.ctypes.data
        lo.x_traj, lo.u_traj, lo.status_traj, lo.iter_traj, lo.xhat_traj, lo.y_traj = (o.ctypes.data for o in out)
        for k, v in change.items():
            setattr(lo, k, v)
        return lo
    mt = _lib.ModelTraj(); mt.struct_size, mt.hold, mt.nmodels, mt.Ad, mt.Bd = C.sizeof(_lib.ModelTraj), hold, Adt.shape[0], Adt.ctypes.data, Bdt.ctypes.data
    et = _lib.EstTraj(); et.struct_size, et.nentries, et.Lgain_traj = C.sizeof(_lib.EstTraj), Lt.shape[0], Lt.ctypes.data
    state = lambda: tuple(bp.iterate_state()) + tuple(bp.scaling()[:3]) + (bp.solution()[0], x_true.copy())
    err = lambda: L.mpcqp_last_error().decode()

    def refused(lo, ms, es):
        """The return codes of loop and taped rollout, which agree, and nothing of the iterate, the solution, the scaling or x_true has changed."""
        before = state()
        codes = [call(h, K, C.byref(lo), None if ms is None else C.byref(ms), None if es is None else C.byref(es)) for call in (L.mpcqp_mpc_loop_tv_est, L.mpcqp_rollout_tv_est)]
        for a, b in zip(before, state()):
            assert np.array_equal(a, b)
        assert codes[0] == codes[1], codes
        return codes[0]

    def copy(s, **change):
        n = type(s)()
        C.memmove(C.byref(n), C.byref(s), C.sizeof(s))
        for k, v in change.items():
            setattr(n, k, v)
        return n
    assert refused(loop(), None, et) == -1                 # no schedule
    for change in (dict(struct_size=8), dict(hold=0), dict(nmodels=2), dict(Ad=None, Bd=None)):      # what mpcqp_mpc_loop_tv refuses
        assert refused(loop(), copy(mt, **change), et) == -1, change
    assert refused(loop(ny=0), mt, et) == -1 and 'ny' in err()                        # no estimator
    assert refused(loop(), mt, copy(et, nentries=2)) == -1 and 'gain entries' in err()
    assert refused(loop(), mt, copy(et, struct_size=8)) == -1
    assert refused(loop(C=None), mt, et) == -1 and refused(loop(x_true=None), mt, et) == -1       # what the output-feedback loop refuses
    assert refused(loop(Lgain=None), mt, None) == -1                                   # no gain at all ...
    assert L.mpcqp_rollout_tv_est(h, K, C.byref(loop(Lgain=None)), C.byref(mt), C.byref(et)) == 0       # ... but a gain schedule stands in for io->Lgain
    Kf = rd.ctrl(name, seeds=seeds)
    want = Kf.run(K, estimator=rd.estimator(Kf, e), model_traj=sched, L_traj=Lt)
    assert np.array_equal(out[4], want['xhat']) and np.array_equal(out[1], want['u']) and np.array_equal(x_true, want['x'][-1])
    n = C.c_int64()
    assert L.mpcqp_rollout_tv_est_tape_bytes(h, K, 0, ny, C.byref(n)) == -1 and L.mpcqp_rollout_tv_est_tape_bytes(h, K, hold, 0, C.byref(n)) == -1
    # the older calls keep refusing the combination, and say where it is
    for call in (L.mpcqp_mpc_loop_tv, L.mpcqp_rollout_tv):
        assert call(h, K, C.byref(loop()), C.byref(mt)) == -4 and 'output feedback' in err() and '_est' in err()
    with pytest.raises(NotImplementedError):
        bp.mpc_run(K, model_traj=sched, estimator=dict(C=e['C'], L=e['L'], x_true=x_true))
    # what mpcqp_rollout refuses, of the taped call alone
    Kt.update(Kt.x0, solve=False)
    before = state()
    assert L.mpcqp_rollout_tv_est(h, K, C.byref(loop()), C.byref(mt), C.byref(et)) == -5      # no solve behind the step data
    for a, b in zip(before, state()):
        assert np.array_equal(a, b)
    Kt.solve()
    bp.update_settings(polish=True)
    assert refused(loop(), mt, et) == -4                   # polishing inside the loop
    bp.update_settings(polish=False)
    assert L.mpcqp_rollout_release(h) == 0

    # every sweep on every kind of tape
    def sweeps():
        io = _lib.RolloutAdjointIO(); io.struct_size = C.sizeof(_lib.RolloutAdjointIO); io.G_x, io.G_u = g['g_x'].ctypes.data, g['g_u'].ctypes.data
        lam = np.empty((K + 1, 2, nx)); io.lam = lam.ctypes.data
        eo = _lib.RolloutEstIO(); eo.struct_size = C.sizeof(_lib.RolloutEstIO)
        bo = _lib.AdjointBoundsIO(); bo.struct_size = C.sizeof(_lib.AdjointBoundsIO)
        to = _lib.RolloutTVIO(); to.struct_size = C.sizeof(_lib.RolloutTVIO)
        xo = _lib.RolloutTVEstIO(); xo.struct_size = C.sizeof(_lib.RolloutTVEstIO)
        return dict(plain=L.mpcqp_rollout_adjoint(h, C.byref(io), None), est=L.mpcqp_rollout_adjoint_est(h, C.byref(io), C.byref(eo), None),
                    bounds=L.mpcqp_rollout_adjoint_bounds(h, C.byref(io), None, None, C.byref(bo)),
                    tv=L.mpcqp_rollout_adjoint_tv(h, C.byref(io), None, None, C.byref(to)),
                    tv_est=L.mpcqp_rollout_adjoint_tv_est(h, C.byref(io), C.byref(eo), None, C.byref(bo), C.byref(to), C.byref(xo)))
    assert set(sweeps().values()) == {-5}                  # no tape
    est = lambda: rd.estimator(Kt, e)
    Kt.rollout(K)
    assert sweeps() == dict(plain=0, est=-5, bounds=0, tv=-5, tv_est=-5)
    with pytest.raises(RuntimeError, match='rollout_tv_est'):
        Kt.rollout_adjoint(g_x=g['g_x'], want=('L_traj',))
    with pytest.raises(RuntimeError, match=r'\(-5\)'):
        bp.rollout_tv_est_gain(0)
    Kt.rollout_est(K, est())
    assert sweeps() == dict(plain=0, est=0, bounds=0, tv=-5, tv_est=-5)
    with pytest.raises(RuntimeError, match='rollout_tv_est'):
        Kt.rollout_adjoint(g_x=g['g_x'], want=('Ae_traj',))
    Kt.rollout_tv(K, sched)
    assert sweeps() == dict(plain=-5, est=-5, bounds=-5, tv=0, tv_est=-5)
    with pytest.raises(RuntimeError, match='rollout_tv_est'):
        Kt.rollout_adjoint(g_x=g['g_x'], want=('Be_traj',))
    with pytest.raises(RuntimeError, match=r'\(-5\)'):
        bp.rollout_tv_est_gain(0)
    Kt.rollout_tv_est(K, sched, est(), L_traj=Lt)
    assert sweeps() == dict(plain=-5, est=-5, bounds=-5, tv=-5, tv_est=0)
    io = _lib.RolloutAdjointIO(); io.struct_size = C.sizeof(_lib.RolloutAdjointIO); io.G_x = g['g_x'].ctypes.data
    assert L.mpcqp_rollout_adjoint(h, C.byref(io), None) == -5 and 'mpcqp_rollout_adjoint_tv_est' in err()
    ref = Kt.rollout_adjoint(want=ALL, **g)
    assert np.all(ref['status'] == 1)
    # the arguments of the new sweep
    buf = np.empty((2, nx, nx))
    for field in ('d_L', 'd_Ae', 'd_Be'):
        eo = _lib.RolloutEstIO(); eo.struct_size = C.sizeof(_lib.RolloutEstIO); setattr(eo, field, buf.ctypes.data)
        assert L.mpcqp_rollout_adjoint_tv_est(h, C.byref(io), C.byref(eo), None, None, None, None) == -1, field
    for field in ('d_Ap', 'd_Bp'):
        bad = copy(io, **{field: buf.ctypes.data})
        assert L.mpcqp_rollout_adjoint_tv_est(h, C.byref(bad), None, None, None, None, None) == -1, field
    short = _lib.RolloutTVEstIO(); short.struct_size = 8
    assert L.mpcqp_rollout_adjoint_tv_est(h, C.byref(io), None, None, None, None, C.byref(short)) == -1
    none = _lib.RolloutAdjointIO(); none.struct_size = C.sizeof(_lib.RolloutAdjointIO)
    assert L.mpcqp_rollout_adjoint_tv_est(h, C.byref(none), None, None, None, None, None) == -1             # no seed
    eo = _lib.RolloutEstIO(); eo.struct_size = C.sizeof(_lib.RolloutEstIO); eo.G_y = g['g_y'].ctypes.data
    assert L.mpcqp_rollout_adjoint_tv_est(h, C.byref(none), C.byref(eo), None, None, None, None) == 0       # (G_y alone is one)
    # the tape is a copy; what invalidates it
    Kt.step(Kt.x0_rh * 0.9)
    again = Kt.rollout_adjoint(want=ALL, **g)
    for k in ALL + ('n_factor',):
        assert np.array_equal(again[k], ref[k]), k
    Kt.update_model(Ad=Kt.Ad * 0.99)
    with pytest.raises(RuntimeError, match=r'\(-5\)'):
        Kt.rollout_adjoint(**g)
    with pytest.raises(ValueError):
        Kt.rollout_tv_est(K, None, est())
    with pytest.raises(ValueError):
        Kt.run(K, model_traj=sched, L_traj=Lt)


# ---- 8. torch ------------------------------------------------------------------------------------------------------------------------------
def test_mpc_rollout_tv_est_is_one_sweep_with_the_matching_seeds():
    import torch
    from pympc_amd.torch_layer import mpc_rollout_tv_est
    name, hold = xc.FIRST, 2
    c = rc.CASES[name]
    K, nx, nu = c['K'], c['nx'], c['nu']
    io = _inputs(name, hold, True, True)
    e, Adt, Bdt, Lt = io['e'], io['Adt'], io['Bdt'], io['Lt']
    dev = torch.device('cuda:0')
    t = lambda a, g=True: torch.tensor(np.asarray(a, dtype=float), dtype=torch.float64, device=dev, requires_grad=g)
    C1 = _ctrl(name)
    B = C1.B
    s = {k: torch.tensor(v, device=dev) for k, v in _seeds(name).items()}
    loss_of = lambda X, XH, Y, U: 0.5 * ((s['g_x'] * X * X).sum() + (s['g_xhat'] * XH * XH).sum() + (s['g_y'] * Y * Y).sum() + (s['g_u'] * U * U).sum())
    # its own plant, noise, a gain per entry, params and bounds beside the schedule
    tx, txh, tC, tv, tu, tw, tA, tB, tAt, tBt, tLt = (t(a) for a in (e['x_true0'], C1.x0, e['C'], io['v'], C1.uminus1, io['w'], io['Ap'], io['Bp'], Adt, Bdt, Lt))
    params, bounds = dict(Ad=t(C1.Ad), Qx=t(C1.Qx[0])), dict(umax=t(C1.umax))
    X, XH, Y, U = mpc_rollout_tv_est(C1, tx, txh, K, tAt, tBt, hold, tC, L_traj=tLt, v=tv, u_prev=tu, w=tw, Ap=tA, Bp=tB, params=params, bounds=bounds)
    assert X.shape == (K + 1, B, nx) and XH.shape == X.shape and U.shape == (K, B, nu) and Y.shape[:2] == (K, B) and X.is_cuda
    ins = [tx, txh, tC, tv, tu, tw, tA, tB, tAt, tBt, tLt, params['Ad'], params['Qx'], bounds['umax']]
    grads = torch.autograd.grad(loss_of(X, XH, Y, U), ins)
    assert np.array_equal(C1.Ad, Adt[-1]) and np.array_equal(C1.Bd, Bdt[-1])         # the controller is left with the last entry
    C2 = _ctrl(name)                                       # the same forward without torch, and the sweep with the seeds the loss implies
    C2.update_model(Ad=C2.Ad, Qx=np.broadcast_to(C2.Qx[0], C2.Qx.shape), umax=C2.umax, solve=False)
    C2.update(C2.x0, C2.uminus1, C2.xref)
    r = C2.rollout_tv_est(K, (Adt, Bdt, hold), rd.estimator(C2, e, v=io['v']), L_traj=Lt, w=io['w'], Ap=io['Ap'], Bp=io['Bp'])
    for o, k in ((X, 'x'), (XH, 'xhat'), (Y, 'y'), (U, 'u')):
        assert np.array_equal(o.detach().cpu().numpy(), r[k]), k
    sn = {k: v.cpu().numpy() for k, v in s.items()}
    ref = C2.rollout_adjoint(g_x=sn['g_x'] * r['x'], g_xhat=sn['g_xhat'] * r['xhat'], g_y=sn['g_y'] * r['y'], g_u=sn['g_u'] * r['u'],
                             want=BASE + TRAJ + ('Ad', 'Ap', 'Bp', 'Qx', 'umax'))
    want = [ref['lam'][0], ref['eta'][0], ref['C'], ref['v'], ref['uminus1'], ref['lam'][1:], ref['Ap'], ref['Bp'], ref['Ad_traj'] + ref['Ae_traj'],
            ref['Bd_traj'] + ref['Be_traj'], ref['L_traj'], ref['Ad'], ref['Qx'].sum(axis=0), ref['umax']]
    for gr, w_, n in zip(grads, want, ('x0', 'xhat0', 'C', 'v', 'u_prev', 'w', 'Ap', 'Bp', 'Ad_traj', 'Bd_traj', 'L_traj', 'Ad', 'Qx', 'umax')):
        assert tuple(gr.shape) == tuple(np.shape(w_)) and gr.is_cuda, n
        assert _rel(gr.cpu().numpy(), w_) <= 1e-13, (n, _rel(gr.cpu().numpy(), w_))
    # the plant follows the schedule; an unbatched schedule, gain schedule and C are reduced through the batch sum
    C3 = _ctrl(name)
    uA, uB, uL, uC = t(Adt[:, 0]), t(Bdt[:, 0]), t(Lt[:, 0]), t(e['C'][0])
    X, XH, Y, U = mpc_rollout_tv_est(C3, t(e['x_true0'], False), t(C1.x0, False), K, uA, uB, hold, uC, L_traj=uL)
    gA, gB, gL, gC = torch.autograd.grad(loss_of(X, XH, Y, U), [uA, uB, uL, uC])
    sd = dict(g_x=(s['g_x'] * X).detach(), g_xhat=(s['g_xhat'] * XH).detach(), g_y=(s['g_y'] * Y).detach(), g_u=(s['g_u'] * U).detach())
    seen = C3.prob.rollout_adjoint(want=TRAJ + ('C',), batch_sum=True, **sd)
    assert seen['L_traj'].is_cuda and seen['L_traj'].shape == (-(-K // hold), 1, nx, Lt.shape[-1])      # device in, device out
    assert torch.equal(gA, (seen['Ad_traj'] + seen['Ae_traj'] + seen['Ap_traj'])[:, 0]) and torch.equal(gB, (seen['Bd_traj'] + seen['Be_traj'] + seen['Bp_traj'])[:, 0])
    assert torch.equal(gL, seen['L_traj'][:, 0]) and torch.equal(gC, seen['C'].sum(dim=0))
    assert float(seen['Ae_traj'].abs().max()) > 1e-3 and float(gL.abs().max()) > 1e-3
    # one constant gain and a schedule of Ad alone: L gets the sum over the entries, params' Bd every slot, the estimator's and the plant's path
    C4 = _ctrl(name)
    pB, tAt, tL = t(C4.Bd), t(Adt), t(e['L'])
    X, XH, Y, U = mpc_rollout_tv_est(C4, t(e['x_true0'], False), t(C1.x0, False), K, tAt, None, hold, t(e['C'], False), L=tL, params=dict(Bd=pB))
    gB, gAt, gL = torch.autograd.grad(loss_of(X, XH, Y, U), [pB, tAt, tL])
    sd = dict(g_x=(s['g_x'] * X).detach(), g_xhat=(s['g_xhat'] * XH).detach(), g_y=(s['g_y'] * Y).detach(), g_u=(s['g_u'] * U).detach())
    r4 = C4.prob.rollout_adjoint(want=('Bd', 'Bp', 'Be', 'Ad_traj', 'Ap_traj', 'Ae_traj', 'L', 'L_traj'), **sd)
    assert _rel(gB.cpu().numpy(), (r4['Bd'] + r4['Bp'] + r4['Be']).cpu().numpy()) <= 1e-13
    assert _rel(gAt.cpu().numpy(), (r4['Ad_traj'] + r4['Ap_traj'] + r4['Ae_traj']).cpu().numpy()) <= 1e-13
    assert _rel(gL.cpu().numpy(), r4['L'].cpu().numpy()) <= 1e-13 and _rel(r4['L'].cpu().numpy(), r4['L_traj'].sum(dim=0).cpu().numpy()) <= 1e-13
    # a second rollout between forward and backward; exactly one of L and L_traj
    X, XH, Y, U = mpc_rollout_tv_est(C4, t(e['x_true0']), t(C1.x0), K, tAt, None, hold, t(e['C'], False), L=tL)
    C4.rollout(2)
    with pytest.raises(RuntimeError, match='rolled out again'):
        XH.sum().backward()
    for kw in (dict(), dict(L=tL, L_traj=t(Lt))):
        with pytest.raises(ValueError):
            mpc_rollout_tv_est(C4, t(e['x_true0']), t(C1.x0), K, tAt, None, hold, t(e['C'], False), **kw)


def test_mpc_rollout_tv_est_on_the_controllers_stream_and_a_kalman_gain_per_entry():
    """Every pointer of the two library calls is a device pointer: forward and backward are stream-ordered on torch's stream.  The gain of
    every entry comes from torch_layer.kalman_gain, so the gradient arrives at the noise covariances."""
    import torch
    from pympc_amd.torch_layer import mpc_rollout_tv_est, kalman_gain
    name, hold = xc.FIRST, 2
    K = rc.CASES[name]['K']
    io = _inputs(name, hold, False, True)
    e, Adt, Bdt = io['e'], io['Adt'], io['Bdt']
    nseg, B, nx = Adt.shape[:3]
    ny = e['C'].shape[1]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        C1 = _ctrl(name, over=dict(stream=stream.cuda_stream))
        dev = torch.device('cuda:0')
        t = lambda a, g=False: torch.tensor(np.asarray(a, dtype=float), dtype=torch.float64, device=dev, requires_grad=g)
        txh, tA, tB, tC = t(C1.x0, True), t(Adt), t(Bdt), t(e['C'])
        Qn, Rn = t(xc.NOISE * np.eye(nx), True), t(xc.NOISE * np.eye(ny), True)
        Lg, _ = kalman_gain(tA.reshape(nseg * B, nx, nx), tC.repeat(nseg, 1, 1), Qn, Rn)
        tL = Lg.reshape(nseg, B, nx, ny)
        assert _rel(tL.detach().cpu().numpy(), io['Lt']) <= 1e-9       # (the table's gains, from the host design)
        seen = []
        orig = C1.prob.rollout_adjoint

        def spy(**kw):
            seen.append(all(v is None or (hasattr(v, 'is_cuda') and v.is_cuda) for v in (kw.get('g_x'), kw.get('g_u'), kw.get('g_xhat'), kw.get('g_y'))))
            res = orig(**kw)
            seen.append(all(v.is_cuda for v in res.values()))
            return res
        C1.prob.rollout_adjoint = spy
        X, XH, Y, U = mpc_rollout_tv_est(C1, t(e['x_true0']), txh, K, tA, tB, hold, tC, L_traj=tL, v=t(io['v']), w=t(io['w']))
        assert 'Ad' in C1._on_device and 'Ad' not in C1.__dict__      # (the last entry stays on the device until somebody reads the attribute)
        tL.retain_grad()
        ((XH[-1] - X[-1]) ** 2).sum().backward()
        assert seen == [True, True] and txh.grad.is_cuda and Qn.grad.is_cuda and tuple(Qn.grad.shape) == (nx, nx) and tuple(Rn.grad.shape) == (ny, ny)
    stream.synchronize()
    C2 = _ctrl(name)
    t2 = C2.rollout_tv_est(K, (Adt, Bdt, hold), rd.estimator(C2, e, v=io['v']), L_traj=tL.detach().cpu().numpy(), w=io['w'])
    d = 2 * (t2['xhat'][-1] - t2['x'][-1])
    gxh, gx = np.zeros_like(t2['xhat']), np.zeros_like(t2['x'])
    gxh[-1], gx[-1] = d, -d
    ref = C2.rollout_adjoint(g_x=gx, g_xhat=gxh, want=('eta', 'L_traj'))
    assert _rel(txh.grad.cpu().numpy(), ref['eta'][0]) <= 1e-13 and _rel(tL.grad.cpu().numpy(), ref['L_traj']) <= 1e-13
    assert float(Qn.grad.abs().max()) > 1e-6 and float(Rn.grad.abs().max()) > 1e-6
    # ... and it is the gradient: a central difference in the scale of Qn through kalman_gain on the host-side loop
    h = 1e-4

    def loss(q):
        with torch.no_grad():
            Lq, _ = kalman_gain(t(Adt).reshape(nseg * B, nx, nx), t(e['C']).repeat(nseg, 1, 1), t(q * xc.NOISE * np.eye(nx)), t(xc.NOISE * np.eye(ny)))
        Kf = _ctrl(name)
        r = Kf.run(K, estimator=rd.estimator(Kf, e, v=io['v']), model_traj=(Adt, Bdt, hold), L_traj=Lq.reshape(nseg, B, nx, ny).cpu().numpy(), w=io['w'])
        return float(((r['xhat'][-1] - r['x'][-1]) ** 2).sum())
    fd = (loss(1.0 + h) - loss(1.0 - h)) / (2 * h)
    an = float((Qn.grad.cpu().numpy() * xc.NOISE * np.eye(nx)).sum())
    print('ROLLOUT_TV_EST_NOISE d/dscale(Qn): sweep + Riccati adjoint %+.6e, central difference %+.6e' % (an, fd))
    assert abs(an - fd) <= FD_TOL * max(1.0, abs(fd))


# ---- 9. the example --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_learn_noise_example_recovers_it():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'learn_noise_through_scheduled_observer.py'), '--batch', '16', '--steps', '12', '--iters', '8'],
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout)
    loss = [float(v) for v in re.findall(r'^iteration +\d+: loss ([0-9.e+-]+)', r.stdout, flags=re.M)]
    assert len(loss) >= 3 and loss[-1] < 1e-2 * loss[0], loss
    m = re.search(r'^parameter: true ([0-9.e+-]+) start ([0-9.e+-]+) learned ([0-9.e+-]+)', r.stdout, flags=re.M)
    true, start, learned = (float(v) for v in m.groups())
    assert abs(learned - true) <= 0.1 * abs(start - true), (true, start, learned)
