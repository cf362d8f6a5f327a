"""The taped rollout under a model schedule and its reverse sweep on the device (include_ext/mpcqp_rollout_tv.h,
pympc_amd/csrc/mpcqp_rollout.h: k_rollout_adjoint_tv) on the closed loops of tests/rollout_tv_cases.py: the trajectories and the handle
against run(model_traj=), bit for bit; the tape and the model slots against a twin stepped on the host; the sweep against the numpy
restatement tests/rollout_tv_ref.py evaluated on the device's own tape and slots; determinism; a constant schedule against the unscheduled
rollout; central differences of run(model_traj=) itself; the refusals; torch; the bits of the unscheduled sweep; the example.

Everything is solved at the project's parity setting eps_abs = eps_rel = 1e-9 (one comparison of section 5 also without equilibration, from cold
starts and with a fixed rho: it says why).  TOL and FD_TOL are those of tests/rollout_dev.py."""
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
import rollout_tv_cases as tc
import rollout_tv_ref as tr
from rollout_dev import TOL, FD_TOL, SOLVED, CHAIN, ctrl as _ctrl, inputs as _inputs
from util import rel1_any as _rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WEIGHTS = tr.WEIGHT_NAMES
BOUNDS = bounds_ref.NAMES
TRAJ = ('Ad_traj', 'Bd_traj', 'Ap_traj', 'Bp_traj')
BASE = ('lam', 'uminus1', 'uref', 'xref')                  # what the schedule leaves as it was in rollout_adjoint's dict
NAMES = tc.NAMES


def _io(name, own_plant, noisy):
    io = _inputs(name, own_plant, noisy)
    return {k: io[k] for k in ('Ap', 'Bp', 'w', 'xref_traj')}


def _slot_parts(name, blob):
    """(Ad [B, nx, nx], Bd [B, nx, nu], the rest [B, ..]) of a slot's model blob."""
    nx, nu = rc.CASES[name]['nx'], rc.CASES[name]['nu']
    B = blob.shape[0]
    return blob[:, :nx * nx].reshape(B, nx, nx), blob[:, nx * nx:nx * nx + nx * nu].reshape(B, nx, nu), blob[:, nx * nx + nx * nu:]


_fwd = {}


def _forward(name, hold, own_plant=False, noisy=False):
    """One forward variant of a case under its schedule, made once: rollout_tv(K) on one controller, its tape and its slots.  The reference
    every test of the variant shares; nobody changes it."""
    key = (name, hold, own_plant, noisy)
    if key not in _fwd:
        K = rc.CASES[name]['K']
        io = _io(name, own_plant, noisy)
        Adt, Bdt = tc.batch_schedule(name, hold)
        Kb = _ctrl(name)
        res = Kb.rollout_tv(K, (Adt, Bdt, hold), **io)
        nseg = tc.nseg(name, hold)
        _fwd[key] = dict(Kb=Kb, tr=res, io=io, sched=(Adt, Bdt), nseg=nseg, tape=[Kb.prob.rollout_tape(k) for k in range(K)],
                         slots=[Kb.prob.rollout_tv_slot(s) for s in range(nseg + 1)], bmaps={})
    return _fwd[key]


def _twin(name, hold, io):
    """The loop written on the host: per step, what the handle holds, then at a boundary update_model(entry, solve=False), then run(1).
    (controller, the K results, what was held before each step, the scaling and model after each update_model)."""
    K = rc.CASES[name]['K']
    Adt, Bdt = tc.batch_schedule(name, hold)
    Ka = _ctrl(name)
    seq, held = [], []
    models = [dict(zip(('D', 'E', 'c'), Ka.prob.scaling()[:3]), Ad=Ka.Ad.copy(), Bd=Ka.Bd.copy())]
    um1, xref = np.array(Ka.uminus1), np.array(Ka.xref).reshape(Ka.B, -1)
    for k in range(K):
        x, z, y = Ka.prob.iterate_state()
        held.append(dict(x=x, z=z, y=y, status=np.array([i.status for i in Ka.prob.infos()]), um1=um1.copy(), xref=xref.copy()))
        if k % hold == 0:
            Ka.update_model(Ad=Adt[k // hold], Bd=Bdt[k // hold], solve=False)
            models.append(dict(zip(('D', 'E', 'c'), Ka.prob.scaling()[:3]), Ad=Adt[k // hold], Bd=Bdt[k // hold]))
        t = Ka.run(1, w=None if io['w'] is None else io['w'][k:k + 1], Ap=io['Ap'], Bp=io['Bp'])
        held[-1]['x0'] = t['x'][0].copy()
        seq.append(t)
        um1 = t['u'][0].copy()
    return Ka, seq, held, models


def _ref_tape(f, name, b):
    nx, nu = rc.CASES[name]['nx'], rc.CASES[name]['nu']
    return [dict(x=e['x'][b], z=e['z'][b], y=e['y'][b], x0=e['step'][b, :nx], um1=e['step'][b, nx:nx + nu], xref=e['step'][b, nx + nu:],
                 solved=bool(e['status'][b] == SOLVED)) for e in f['tape']]


def _ref_slots(f, name, b):
    out = []
    for s in f['slots']:
        Ad, Bd, _ = _slot_parts(name, s['model'])
        out.append(dict(Ad=Ad[b], Bd=Bd[b], D=s['D'][b], E=s['E'][b], c=s['c'][b]))
    return out


def _reference(f, name, hold, b, gx, gu):
    """The restatement's sweep of instance b on the device's tape and slots."""
    kw, attrs = rc.draw(name, rc.CASES[name]['seeds'][b])
    tape = _ref_tape(f, name, b)
    if b not in f['bmaps']:
        f['bmaps'][b] = bounds_ref.bound_maps(rr.entry_kwargs(kw, tape[0]), attrs)
    io = f['io']
    return tr.sweep(kw, attrs, tape, _ref_slots(f, name, b), hold, None if gx is None else gx[:, b], None if gu is None else gu[:, b],
                    Ap=None if io['Ap'] is None else io['Ap'][b], Bp=None if io['Bp'] is None else io['Bp'][b], bmaps=f['bmaps'][b])


def _seeds(name, B=None):
    c = rc.CASES[name]
    B = len(c['seeds']) if B is None else B
    rng = np.random.default_rng(31)
    return rng.standard_normal((c['K'] + 1, B, c['nx'])), rng.standard_normal((c['K'], B, c['nu']))


def _slot_sums(got, ref, b):
    """(name, device value, restatement's) of the four per-entry outputs and of 'Ad', 'Bd', 'Ap', 'Bp' as rollout_adjoint puts them together
    for a schedule that gave both matrices."""
    return [('Ad_traj', got['Ad_traj'][:, b], ref['Ad_slots'][1:]), ('Bd_traj', got['Bd_traj'][:, b], ref['Bd_slots'][1:]),
            ('Ap_traj', got['Ap_traj'][:, b], ref['Ap_entries']), ('Bp_traj', got['Bp_traj'][:, b], ref['Bp_entries']),
            ('Ad', got['Ad'][b], ref['Ad_slots'][0]), ('Bd', got['Bd'][b], ref['Bd_slots'][0]),
            ('Ap', got['Ap'][b], ref['Ap_entries'].sum(axis=0)), ('Bp', got['Bp'][b], ref['Bp_entries'].sum(axis=0))]


ALL = BASE + TRAJ + ('Ad', 'Bd', 'Ap', 'Bp') + WEIGHTS + BOUNDS


# ---- 1. forward against the loop -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hold', ('1', '2', 'K+1'))
@pytest.mark.parametrize('name', NAMES)
def test_rollout_tv_is_run_with_the_schedule(name, hold):
    K = rc.CASES[name]['K']
    hold = K + 1 if hold == 'K+1' else int(hold)
    for own_plant, noisy in ((False, False), (True, True)):
        io = _io(name, own_plant, noisy)
        if hold <= 2:
            f = _forward(name, hold, own_plant, noisy)
            Kb, got, (Adt, Bdt) = f['Kb'], f['tr'], f['sched']
        else:                                              # one entry for the whole loop
            Adt, Bdt = tc.batch_schedule(name, hold)
            assert Adt.shape[0] == 1
            Kb = _ctrl(name)
            got = Kb.rollout_tv(K, (Adt, Bdt, hold), **io)
        Kd = _ctrl(name)
        want = Kd.run(K, model_traj=(Adt, Bdt, hold), **io)
        for k in ('x', 'u', 'status', 'iter'):
            assert np.array_equal(got[k], want[k]), (name, hold, k)
        assert np.all(got['status'] == SOLVED)
        for va, vb in zip(Kb.prob.iterate_state(), Kd.prob.iterate_state()):
            assert np.array_equal(va, vb), (name, hold)
        (xa, ya, ia), (xb, yb, ib) = Kb.prob.solution(), Kd.prob.solution()
        assert np.array_equal(xa, xb) and np.array_equal(ya, yb) and [bytes(i) for i in ia] == [bytes(i) for i in ib], (name, hold)
        last = (K - 1) // hold
        assert np.array_equal(Kb.Ad, Adt[last]) and np.array_equal(Kb.Bd, Bdt[last]) and np.array_equal(Kd.Ad, Kb.Ad) and np.array_equal(Kd.Bd, Kb.Bd)
        assert np.array_equal(Kb.uminus1_rh, Kd.uminus1_rh) and np.array_equal(Kb.x0_rh, Kd.x0_rh)
        if not own_plant:                                  # the plant followed the model in force
            for k in range(K):
                xn = np.einsum('bij,bj->bi', Adt[k // hold], got['x'][k]) + np.einsum('bij,bj->bi', Bdt[k // hold], got['u'][k])
                assert np.allclose(xn, got['x'][k + 1], rtol=1e-13, atol=1e-14)


# ---- 2. the tape and the slots against the host --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hold', tc.HOLDS)
@pytest.mark.parametrize('name', NAMES)
def test_the_tape_and_the_slots_are_what_the_handle_held(name, hold):
    nx, nu, K = rc.CASES[name]['nx'], rc.CASES[name]['nu'], rc.CASES[name]['K']
    for own_plant, noisy in ((False, False), (True, True)):
        f = _forward(name, hold, own_plant, noisy)
        Ka, seq, held, models = _twin(name, hold, f['io'])
        for k in range(K):
            for v in ('x', 'u', 'status', 'iter'):
                assert np.array_equal(f['tr'][v][k], seq[k][v][0]), (name, hold, k, v)
            e, h = f['tape'][k], held[k]
            for v in ('x', 'z', 'y', 'status'):
                assert np.array_equal(e[v], h[v]), (name, hold, k, v)
            assert np.array_equal(e['step'][:, :nx], h['x0']) and np.array_equal(e['step'][:, nx:nx + nu], h['um1']), (name, hold, k)
            assert np.array_equal(e['step'][:, nx + nu:], h['xref']), (name, hold, k)
        assert len(f['slots']) == len(models) == f['nseg'] + 1
        rest0 = _slot_parts(name, f['slots'][0]['model'])[2]
        for s, (slot, m) in enumerate(zip(f['slots'], models)):
            Ad, Bd, rest = _slot_parts(name, slot['model'])
            assert np.array_equal(Ad, m['Ad']) and np.array_equal(Bd, m['Bd']), (name, hold, s)
            assert np.array_equal(rest, rest0), (name, hold, s)        # (bounds, uref, eps_feas, weights: the schedule does not touch them)
            for v in ('D', 'E', 'c'):
                assert np.array_equal(slot[v], m[v]), (name, hold, s, v)
        assert not np.array_equal(f['slots'][0]['D'], f['slots'][1]['D'])          # (update_model re-equilibrates)
    fresh = _ctrl(name)                                    # slot 0 is the setup's
    for v, a in zip(('D', 'E', 'c'), fresh.prob.scaling()[:3]):
        assert np.array_equal(f['slots'][0][v], a), v
    Ad0, Bd0, _ = _slot_parts(name, f['slots'][0]['model'])
    assert np.array_equal(Ad0, fresh.Ad) and np.array_equal(Bd0, fresh.Bd)
    bp = f['Kb'].prob
    assert bp.rollout_tv_tape_bytes(K, hold) > bp.rollout_tape_bytes(K) > 0
    with pytest.raises(RuntimeError, match=r'\(-1\)'):
        bp.rollout_tv_slot(f['nseg'] + 1)
    with pytest.raises(RuntimeError, match=r'\(-1\)'):
        bp.rollout_tape(K)


# ---- 3. the reverse sweep against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('own_plant', (False, True), ids=('plant_follows', 'plant_given'))
@pytest.mark.parametrize('hold', tc.HOLDS)
@pytest.mark.parametrize('name', NAMES)
def test_the_sweep_is_the_restatement(name, hold, own_plant):
    f = _forward(name, hold, own_plant, own_plant)
    Kb, K, nseg = f['Kb'], rc.CASES[name]['K'], f['nseg']
    gx, gu = _seeds(name)
    got = Kb.rollout_adjoint(g_x=gx, g_u=gu, want=ALL)
    nact, nweak, status, nfac = Kb.prob.rollout_info()
    assert np.all(status == 1) and np.all(nweak == 0), (name, status, nweak)
    assert got['Ad_traj'].shape == (nseg, Kb.B, Kb.nx, Kb.nx) and got['Bp_traj'].shape == (nseg, Kb.B, Kb.nx, Kb.nu)
    errs = {}
    for b in range(Kb.B):
        ref = _reference(f, name, hold, b, gx, gu)
        assert np.array_equal(nact[:, b], ref['n_active']) and np.array_equal(nweak[:, b], ref['n_weak']), (name, b, nact[:, b], ref['n_active'])
        assert nfac[b] == ref['n_factor'], (name, hold, b, nfac[b], ref['n_factor'])
        pairs = [(k, got[k][:, b] if k in ('lam', 'xref') else got[k][b], ref[k]) for k in BASE + WEIGHTS + BOUNDS] + _slot_sums(got, ref, b)
        for k, v, r in pairs:
            errs[k] = max(errs.get(k, 0.0), _rel(v, r))
        if hold == 1:                                      # the last entry's only solve is the one for x_K, which is on no tape
            assert np.all(got['Ad_traj'][-1, b] == 0.0) and np.all(got['Bd_traj'][-1, b] == 0.0)
            assert np.abs(got['Ap_traj'][-1, b]).max() > 0.0 and np.abs(got['Bp_traj'][-1, b]).max() > 0.0
    worst = max(errs.values())
    print('ROLLOUT_TV_ERR %s hold %d plant %s: max %.3e  %s' % (name, hold, 'given' if own_plant else 'follows', worst, ' '.join('%s=%.1e' % kv for kv in errs.items())))
    assert worst <= TOL, (name, hold, errs)
    assert got['n_factor'].shape == (Kb.B,) and got['status'].shape == (K, Kb.B)


def test_a_slot_change_under_an_equal_active_set_is_a_new_factor():
    """'first' at hold 2 has consecutive entries with equal active sets made under different slots (tests/test_rollout_tv_cases.py): the
    sweep factors there, so it makes more factorizations than the changes of active set alone would ask for."""
    f = _forward(rc.FIRST, 2)
    gx, gu = _seeds(rc.FIRST)
    got = f['Kb'].rollout_adjoint(g_x=gx, g_u=gu, want=('lam',))
    more = []
    for b in range(f['Kb'].B):
        ref = _reference(f, rc.FIRST, 2, b, gx, gu)
        sets = ref['sets']
        by_set = 1 + sum(1 for k in range(len(sets) - 1) if not (np.array_equal(sets[k][0], sets[k + 1][0]) and np.array_equal(sets[k][1], sets[k + 1][1])))
        assert got['n_factor'][b] == ref['n_factor'] >= by_set
        more.append(ref['n_factor'] > by_set)
    assert any(more), more


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ('first', 'held'))
def test_two_sweeps_reuse_and_batch_sum(name):
    f = _forward(name, 2)
    Kb, K = f['Kb'], rc.CASES[name]['K']
    gx, gu = _seeds(name)
    a = Kb.rollout_adjoint(g_x=gx, g_u=gu, want=ALL)
    b = Kb.rollout_adjoint(g_x=gx, g_u=gu, want=ALL)
    c = Kb.rollout_adjoint(g_x=gx, g_u=gu, want=ALL, no_reuse=True)
    for k in ALL + ('n_weak', 'status'):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), (name, k)
    assert np.array_equal(a['n_factor'], b['n_factor']) and np.all(c['n_factor'] == K) and np.all(a['n_factor'] <= K)
    for want in (('Ad_traj',), ('Bd_traj', 'Bp_traj'), ('Bd',)):      # asked for on their own (no weight beside them): the same bits
        d = Kb.rollout_adjoint(g_x=gx, g_u=gu, want=want)
        for k in want:
            assert np.array_equal(d[k], a[k]) and (np.abs(d[k]).max() > 0.0 or not k.endswith('_traj')), (name, want, k)
    s1 = Kb.rollout_adjoint(g_x=gx, g_u=gu, want=TRAJ + ('Ad', 'Bd', 'Ap', 'Bp') + WEIGHTS + BOUNDS, batch_sum=True)
    s2 = Kb.rollout_adjoint(g_x=gx, g_u=gu, want=TRAJ + ('Ad', 'Bd', 'Ap', 'Bp') + WEIGHTS + BOUNDS, batch_sum=True)
    for k in TRAJ:
        assert s1[k].shape[1] == 1 and np.array_equal(s1[k], s2[k]), k
        assert _rel(s1[k][:, 0], a[k].sum(axis=1)) <= 1e-13, k
    for k in ('Ad', 'Bd', 'Ap', 'Bp') + WEIGHTS + BOUNDS:
        assert s1[k].shape[0] == 1 and np.array_equal(s1[k], s2[k]), k
        assert _rel(s1[k][0], a[k].sum(axis=0)) <= 1e-13, k


# ---- 5. a constant schedule is the unscheduled rollout -------------------------------------------------------------------------------------
# update_model of an equal model is not a no-op on the solves that follow: it equilibrates again, and the cost scaling c it arrives at
# depends on q, that is on the state the loop has reached; it leaves rho as adapted but the next solve starts from z = A x
# (mpcqp_update_model).  So under the default settings the scheduled loop reaches the same solutions by other iterates, and the two
# trajectories agree to the solver's tolerance only -- measured on the MI355X, 'first', max over x and u: 2.7e-9 at eps 1e-9, 3.7e-12 at
# 1e-12, 1.7e-13 at 1e-13 (where rows begin to count as weakly active), and no convergence below.  What follows from the active sets alone
# (the chain, the bounds) is held to 1e-13 under the default settings; the model gradients are sums of products with the iterates and the
# trajectory, so they are held to 1e-13 where the two forward loops are the same loop: without equilibration (D = E = c = 1 from any q),
# from a cold start of every solve and with rho fixed, update_model of an equal model changes nothing the solves read.
SAME_LOOP = dict(scaling=0, warm_start=0, adaptive_rho=0)
_const = {}


def _constant(hold, **settings):
    """'first' rolled out on one model and under a schedule whose every entry is that model, and both swept with the same seeds; made once
    per (hold, settings)."""
    key = (hold,) + tuple(sorted(settings.items()))
    if key not in _const:
        name = rc.FIRST
        K = rc.CASES[name]['K']
        nseg = tc.nseg(name, hold)
        io = _io(name, False, True)
        Ku, Kc = _ctrl(name, **settings), _ctrl(name, **settings)
        tu = Ku.rollout(K, **io)
        sched = (np.repeat(Kc.Ad[None], nseg, axis=0), np.repeat(Kc.Bd[None], nseg, axis=0), hold)
        ts = Kc.rollout_tv(K, sched, **io)
        gx, gu = _seeds(name)
        ref = Ku.rollout_adjoint(g_x=gx, g_u=gu, want=CHAIN + ('Ad', 'Bd') + WEIGHTS + BOUNDS)
        got = Kc.rollout_adjoint(g_x=gx, g_u=gu, want=ALL)
        assert np.all(ref['status'] == 1) and np.all(got['status'] == 1)
        print('ROLLOUT_TV_CONST hold %d %s: x %.3e u %.3e' % (hold, settings, _rel(ts['x'], tu['x']), _rel(ts['u'], tu['u'])))
        _const[key] = dict(ref=ref, got=got, io=io, sched=sched, gx=gx, gu=gu, K=K, tu=tu, ts=ts)
    return _const[key]


@pytest.mark.parametrize('hold', tc.HOLDS)
def test_a_constant_schedule_gives_the_unscheduled_chain_and_bounds(hold):
    f = _constant(hold)
    errs = {k: _rel(f['got'][k], f['ref'][k]) for k in BASE + BOUNDS}
    print('ROLLOUT_TV_CONST hold %d: %s' % (hold, ' '.join('%s=%.1e' % kv for kv in errs.items())))
    assert max(errs.values()) <= 1e-13, errs


@pytest.mark.parametrize('hold', tc.HOLDS)
def test_the_slot_sums_of_a_constant_schedule_are_the_unscheduled_model_gradients(hold):
    """The slot sums against the unscheduled rollout's Ad, Bd, Ap, Bp within 1e-13, and with them the chain, the bounds and the weights, under
    SAME_LOOP (see above): there the two forward loops give the same bits, which is asserted first, so that every difference left is the
    sweep's -- its slots, its re-aimed pointers, the factor it drops at every slot change, the order of its sums."""
    f = _constant(hold, **SAME_LOOP)
    got, ref = f['got'], f['ref']
    for k in ('x', 'u', 'status', 'iter'):
        assert np.array_equal(f['ts'][k], f['tu'][k]), k
    errs = dict(Ad=_rel(got['Ad'] + got['Ad_traj'].sum(axis=0), ref['Ad']), Bd=_rel(got['Bd'] + got['Bd_traj'].sum(axis=0), ref['Bd']),
                Ap=_rel(got['Ap_traj'].sum(axis=0), ref['Ap']), Bp=_rel(got['Bp_traj'].sum(axis=0), ref['Bp']))
    errs.update({k: _rel(got[k], ref[k]) for k in BASE + WEIGHTS + BOUNDS})
    print('ROLLOUT_TV_CONST_SUMS hold %d: %s' % (hold, ' '.join('%s=%.1e' % kv for kv in errs.items())))
    assert _rel(got['Ap_traj'].sum(axis=0), got['Ap']) <= 1e-13 and _rel(got['Bp_traj'].sum(axis=0), got['Bp']) <= 1e-13
    assert max(errs.values()) <= 1e-13, errs


def test_a_schedule_of_one_matrix_leaves_the_other_to_the_controller():
    """A schedule that gives Ad alone: 'Bd' never changed, so its gradient is the sum over every slot."""
    f = _constant(2)
    Kd = _ctrl(rc.FIRST)
    Kd.rollout_tv(f['K'], (f['sched'][0], None, 2), **f['io'])
    only = Kd.rollout_adjoint(g_x=f['gx'], g_u=f['gu'], want=('Ad', 'Bd', 'Ad_traj', 'Bd_traj'))
    got = f['got']
    assert _rel(only['Bd'], only['Bd_traj'].sum(axis=0) + got['Bd']) <= 1e-13
    assert np.array_equal(only['Ad'], got['Ad']) and np.array_equal(only['Ad_traj'], got['Ad_traj']) and np.array_equal(only['Bd_traj'], got['Bd_traj'])


# ---- 6. end to end: central differences of run(model_traj=) itself --------------------------------------------------------------------------
def test_the_sweep_against_central_differences_of_the_device_loop():
    """L = sum <Gx[k], x_k> + sum <Gu[k], u_k> of run(K, model_traj=) on fresh controllers, in a direction of x0 and one of the whole Ad
    schedule (the plant follows it: solve path plus plant path).  h as in tests/test_gpu_rollout.py."""
    name, hold = rc.FIRST, 2
    c = rc.CASES[name]
    K, B = c['K'], len(c['seeds'])
    gx, gu = _seeds(name)
    f = _forward(name, hold)
    got = f['Kb'].rollout_adjoint(g_x=gx, g_u=gu, want=('lam', 'Ad_traj', 'Ap_traj'))
    assert np.all(got['status'] == 1) and np.all(got['n_weak'] == 0)
    Adt, Bdt = f['sched']
    base = rc.batch_kwargs(name)
    rng = np.random.default_rng(37)
    h = 1e-4

    def loss(x0, At):
        t = _ctrl(name, over=dict(x0=x0)).run(K, model_traj=(At, Bdt, hold))
        return (gx * t['x']).sum(axis=(0, 2)) + (gu * t['u']).sum(axis=(0, 2))      # per instance: they are independent

    def unit(shape, axis_b):
        d = rng.standard_normal(shape)
        n = np.sqrt((np.moveaxis(d, axis_b, 0).reshape(B, -1) ** 2).sum(axis=1))
        return d / n.reshape([B if i == axis_b else 1 for i in range(d.ndim)])

    d = unit(base['x0'].shape, 0)
    checks = [('x0', (got['lam'][0] * d).sum(axis=1), (loss(base['x0'] + h * d, Adt) - loss(base['x0'] - h * d, Adt)) / (2 * h))]
    d = unit(Adt.shape, 1)
    checks.append(('Ad_traj', ((got['Ad_traj'] + got['Ap_traj']) * d).sum(axis=(0, 2, 3)), (loss(base['x0'], Adt + h * d) - loss(base['x0'], Adt - h * d)) / (2 * h)))
    for field, an, fd in checks:
        err = np.abs(an - fd).max()
        print('ROLLOUT_TV_FD d/d%s: |grad.d - FD|_inf = %.3e, |FD|_inf = %.3e' % (field, err, np.abs(fd).max()))
        assert err <= FD_TOL * max(1.0, np.abs(fd).max()), (field, err, an, fd)
        assert np.abs(fd).max() > 1e-2


# ---- 7. the refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_kind_of_the_tape():
    from pympc_amd import _lib
    name = rc.FIRST
    c = rc.CASES[name]
    K, nx, nu = c['K'], c['nx'], c['nu']
    Kt = _ctrl(name, seeds=(0, 3))
    bp = Kt.prob
    L, h = bp._L, bp._h
    gx, gu = _seeds(name, B=2)
    Adt, Bdt = tc.batch_schedule(name, 2, seeds=(0, 3))
    sched = (Adt, Bdt, 2)
    io = _lib.RolloutAdjointIO(); io.struct_size = C.sizeof(_lib.RolloutAdjointIO); io.G_x, io.G_u = gx.ctypes.data, gu.ctypes.data
    mt = _lib.ModelTraj(); mt.struct_size, mt.hold, mt.nmodels, mt.Ad, mt.Bd = C.sizeof(_lib.ModelTraj), 2, Adt.shape[0], Adt.ctypes.data, Bdt.ctypes.data
    state = lambda: tuple(bp.iterate_state()) + tuple(bp.scaling()[:3]) + (bp.solution()[0],)
    err = lambda: L.mpcqp_last_error().decode()

    def refused(lo, sched_struct):
        """mpcqp_rollout_tv's return code, and nothing of the iterate, the solution or the scaling has changed."""
        before = state()
        code = L.mpcqp_rollout_tv(h, K, C.byref(lo), None if sched_struct is None else C.byref(sched_struct))
        for a, b in zip(before, state()):
            assert np.array_equal(a, b)
        return code
    # what mpcqp_mpc_loop_tv refuses, and no schedule at all
    assert refused(_lib.Loop(), None) == -1 and 'mpcqp_rollout' in err()
    for change, code in ((dict(struct_size=8), -1), (dict(hold=0), -1), (dict(nmodels=2), -1), (dict(Ad=None, Bd=None), -1)):
        bad = _lib.ModelTraj(); C.memmove(C.byref(bad), C.byref(mt), C.sizeof(mt))
        for k, v in change.items():
            setattr(bad, k, v)
        assert refused(_lib.Loop(), bad) == code, change
    lo = _lib.Loop(); lo.ny = 1
    assert refused(lo, mt) == -4                           # output feedback under a schedule
    n = C.c_int64()
    assert L.mpcqp_rollout_tv_tape_bytes(h, K, 0, C.byref(n)) == -1
    # what mpcqp_rollout refuses
    bp.update_settings(polish=True)
    assert refused(_lib.Loop(), mt) == -4                  # polishing inside the loop
    bp.update_settings(polish=False)
    Kt.update(Kt.x0, solve=False)
    assert refused(_lib.Loop(), mt) == -5                  # no solve behind the step data
    Kt.solve()
    before = state()
    with pytest.raises(NotImplementedError):                                          # a time-varying reference of another shape than the controller's
        Kt.rollout_tv(K, sched, xref_traj=np.zeros((K, 2, (c['Np'] + 1) * nx)))
    for a, b in zip(before, state()):
        assert np.array_equal(a, b)
    _, q, _, l, u = bp.export_qp()
    bp.update_vectors(q)
    assert refused(_lib.Loop(), mt) == -5                  # raw-vector mode
    Kt.update(Kt.x0, Kt.uminus1)
    to = _lib.RolloutTVIO(); to.struct_size = C.sizeof(_lib.RolloutTVIO)
    assert L.mpcqp_rollout_adjoint_tv(h, C.byref(io), None, None, C.byref(to)) == -5                    # no tape
    # the kind of the tape
    Kt.rollout(K)
    assert L.mpcqp_rollout_adjoint_tv(h, C.byref(io), None, None, C.byref(to)) == -5 and 'mpcqp_rollout_adjoint' in err()
    with pytest.raises(RuntimeError, match='rollout_tv'):
        Kt.rollout_adjoint(g_x=gx, g_u=gu, want=('Ad_traj',))
    with pytest.raises(RuntimeError, match=r'\(-5\)'):
        bp.rollout_tv_slot(0)
    Kt.rollout_tv(K, sched)
    ref = Kt.rollout_adjoint(g_x=gx, g_u=gu, want=ALL)
    assert np.all(ref['status'] == 1)
    eo = _lib.RolloutEstIO(); eo.struct_size = C.sizeof(_lib.RolloutEstIO)
    bo = _lib.AdjointBoundsIO(); bo.struct_size = C.sizeof(_lib.AdjointBoundsIO)
    lam = np.empty((K + 1, 2, nx)); io.lam = lam.ctypes.data
    for rc_, what in ((L.mpcqp_rollout_adjoint(h, C.byref(io), None), 'mpcqp_rollout_adjoint'),
                      (L.mpcqp_rollout_adjoint_est(h, C.byref(io), C.byref(eo), None), 'mpcqp_rollout_adjoint_est'),
                      (L.mpcqp_rollout_adjoint_bounds(h, C.byref(io), None, None, C.byref(bo)), 'mpcqp_rollout_adjoint_bounds')):
        assert rc_ == -5, what
    assert L.mpcqp_rollout_adjoint(h, C.byref(io), None) == -5 and 'mpcqp_rollout_adjoint_tv' in err()
    # the arguments of the scheduled sweep
    buf = np.empty((2, nx, nx))
    for field in ('d_Ap', 'd_Bp'):
        bad = _lib.RolloutAdjointIO(); C.memmove(C.byref(bad), C.byref(io), C.sizeof(io)); setattr(bad, field, buf.ctypes.data)
        assert L.mpcqp_rollout_adjoint_tv(h, C.byref(bad), None, None, C.byref(to)) == -1, field
    for field in ('d_Ad', 'd_Bd'):
        mo = _lib.AdjointModelIO(); mo.struct_size = C.sizeof(_lib.AdjointModelIO); setattr(mo, field, buf.ctypes.data)
        assert L.mpcqp_rollout_adjoint_tv(h, C.byref(io), C.byref(mo), None, C.byref(to)) == -1, field
    short = _lib.RolloutTVIO(); short.struct_size = 8
    assert L.mpcqp_rollout_adjoint_tv(h, C.byref(io), None, None, C.byref(short)) == -1
    none = _lib.RolloutAdjointIO(); none.struct_size = C.sizeof(_lib.RolloutAdjointIO)
    assert L.mpcqp_rollout_adjoint_tv(h, C.byref(none), None, None, C.byref(to)) == -1                  # no seed
    assert L.mpcqp_rollout_adjoint_tv(h, C.byref(io), None, None, None) == 0                            # (every struct but the seeds' is optional)
    assert np.array_equal(lam, ref['lam'])
    # the tape is a copy: steps and solves in between change no bit of the sweep
    Kt.step(Kt.x0_rh * 0.9)
    again = Kt.rollout_adjoint(g_x=gx, g_u=gu, want=ALL)
    for k in ALL + ('n_factor',):
        assert np.array_equal(again[k], ref[k]), k
    # what invalidates it
    Kt.update_model(Ad=Kt.Ad * 0.99)
    with pytest.raises(RuntimeError, match=r'\(-5\)'):
        Kt.rollout_adjoint(g_x=gx, g_u=gu)
    Kt.rollout_tv(K, sched)
    assert np.all(Kt.rollout_adjoint(g_x=gx, g_u=gu)['status'] == 1)
    _, q, _, l, u = bp.export_qp()
    bp.update_vectors(None, np.clip(l, -1e30, 1e30), np.clip(u, -1e30, 1e30))
    with pytest.raises(RuntimeError, match=r'\(-5\)'):
        Kt.rollout_adjoint(g_x=gx, g_u=gu)
    a = rc.batch_kwargs(name, (0, 3))
    Kt.update(a['x0'], a['uminus1']); Kt.rollout_tv(K, sched)
    bp.setup(a['Ad'], a['Bd'], a['Qx'], a['QxN'], a['Qu'], a['QDu'], a['xmin'], a['xmax'], a['umin'], a['umax'], a['Dumin'], a['Dumax'], a['uref'],
             Kt.eps_feas, a['x0'], a['uminus1'], a['xref'])
    with pytest.raises(RuntimeError, match=r'\(-5\)'):
        Kt.rollout_adjoint(g_x=gx, g_u=gu)
    Kt.solve(); Kt.rollout_tv(K, sched)
    assert np.all(Kt.rollout_adjoint(g_x=gx, g_u=gu)['status'] == 1)
    Kt.rollout(K)                                          # an unscheduled rollout on the same handle: the older sweep again, the new names refused
    assert np.all(Kt.rollout_adjoint(g_x=gx, g_u=gu, want=CHAIN)['status'] == 1)
    bp.rollout_release()
    assert L.mpcqp_rollout_adjoint_tv(h, C.byref(io), None, None, C.byref(to)) == -5
    with pytest.raises(ValueError):
        Kt.rollout_tv(K, None)


# ---- 8. torch ------------------------------------------------------------------------------------------------------------------------------
def test_mpc_rollout_tv_is_one_sweep_with_the_matching_seeds():
    import torch
    from pympc_amd.torch_layer import mpc_rollout_tv
    name, hold = rc.FIRST, 2
    c = rc.CASES[name]
    K, nx, nu = c['K'], c['nx'], c['nu']
    io = _io(name, True, True)
    Adt, Bdt = tc.batch_schedule(name, hold)
    dev = torch.device('cuda:0')
    t = lambda a, g=True: torch.tensor(np.asarray(a, dtype=float), dtype=torch.float64, device=dev, requires_grad=g)
    C1 = _ctrl(name)
    B = C1.B
    wx, wu = torch.tensor(_seeds(name)[0], device=dev), torch.tensor(_seeds(name)[1], device=dev)
    loss_of = lambda X, U: 0.5 * (wx * X * X).sum() + 0.5 * (wu * U * U).sum()
    # its own plant, w, xref, bounds and params beside the schedule
    tx, tu, txr, tw, tA, tB, tAt, tBt = t(C1.x0), t(C1.uminus1), t(C1.xref), t(io['w']), t(io['Ap']), t(io['Bp']), t(Adt), t(Bdt)
    params, bounds = dict(Ad=t(C1.Ad), Qx=t(C1.Qx[0])), dict(umax=t(C1.umax))
    X, U = mpc_rollout_tv(C1, tx, K, tAt, tBt, hold, u_prev=tu, xref=txr, w=tw, Ap=tA, Bp=tB, params=params, bounds=bounds)
    assert X.shape == (K + 1, B, nx) and U.shape == (K, B, nu) and X.is_cuda
    ins = [tx, tu, txr, tw, tA, tB, tAt, tBt, params['Ad'], params['Qx'], bounds['umax']]
    grads = torch.autograd.grad(loss_of(X, U), ins)
    assert np.array_equal(C1.Ad, Adt[-1]) and np.array_equal(C1.Bd, Bdt[-1])         # the controller is left with the last entry
    C2 = _ctrl(name)                                       # the same forward without torch, and the sweep with the seeds the loss implies
    C2.update_model(Ad=C2.Ad, Qx=np.broadcast_to(C2.Qx[0], C2.Qx.shape), umax=C2.umax, solve=False)
    C2.update(C2.x0, C2.uminus1, C2.xref)
    ref_tr = C2.rollout_tv(K, (Adt, Bdt, hold), w=io['w'], Ap=io['Ap'], Bp=io['Bp'])
    assert np.array_equal(X.detach().cpu().numpy(), ref_tr['x']) and np.array_equal(U.detach().cpu().numpy(), ref_tr['u'])
    gx, gu = wx.cpu().numpy() * ref_tr['x'], wu.cpu().numpy() * ref_tr['u']
    ref = C2.rollout_adjoint(g_x=gx, g_u=gu, want=BASE + TRAJ + ('Ad', 'Ap', 'Bp', 'Qx', 'umax'))
    want = [ref['lam'][0], ref['uminus1'], ref['xref'].sum(axis=0), ref['lam'][1:], ref['Ap'], ref['Bp'], ref['Ad_traj'], ref['Bd_traj'], ref['Ad'],
            ref['Qx'].sum(axis=0), ref['umax']]
    for g, w_, n in zip(grads, want, ('x0', 'u_prev', 'xref', 'w', 'Ap', 'Bp', 'Ad_traj', 'Bd_traj', 'Ad', 'Qx', 'umax')):
        assert tuple(g.shape) == tuple(np.shape(w_)) and g.is_cuda, n
        assert _rel(g.cpu().numpy(), w_) <= 1e-13, (n, _rel(g.cpu().numpy(), w_))
    # the plant follows the schedule: entry e gets its plant path too; an unbatched schedule is reduced through the batch sum
    C3 = _ctrl(name)
    uA, uB = t(Adt[:, 0]), t(Bdt[:, 0])
    X, U = mpc_rollout_tv(C3, t(C1.x0, False), K, uA, uB, hold)
    gA, gB = torch.autograd.grad(loss_of(X, U), [uA, uB])
    gxd, gud = (wx * X).detach(), (wu * U).detach()
    seen = C3.prob.rollout_adjoint(g_x=gxd, g_u=gud, want=TRAJ, batch_sum=True)
    assert seen['Ad_traj'].is_cuda and seen['Ad_traj'].shape == (tc.nseg(name, hold), 1, nx, nx)      # device in, device out
    assert torch.equal(gA, (seen['Ad_traj'] + seen['Ap_traj'])[:, 0]) and torch.equal(gB, (seen['Bd_traj'] + seen['Bp_traj'])[:, 0])
    per = C3.prob.rollout_adjoint(g_x=gxd, g_u=gud, want=('Ad_traj', 'Ap_traj'))
    assert _rel(gA.cpu().numpy(), (per['Ad_traj'] + per['Ap_traj']).sum(dim=1).cpu().numpy()) <= 1e-13
    assert float(seen['Ap_traj'].abs().max()) > 1e-3                               # (a path that is there)
    # a schedule of Ad alone: params' Bd never changed and gets every slot and the whole plant path
    C4 = _ctrl(name)
    pB, tAt = t(C4.Bd), t(Adt)
    X, U = mpc_rollout_tv(C4, t(C1.x0, False), K, tAt, None, hold, params=dict(Bd=pB))
    gB, gAt = torch.autograd.grad(loss_of(X, U), [pB, tAt])
    r4 = C4.prob.rollout_adjoint(g_x=(wx * X).detach(), g_u=(wu * U).detach(), want=('Bd', 'Bp', 'Bd_traj', 'Ad_traj', 'Ap_traj'))
    assert _rel(gB.cpu().numpy(), (r4['Bd'] + r4['Bp']).cpu().numpy()) <= 1e-13 and _rel(gAt.cpu().numpy(), (r4['Ad_traj'] + r4['Ap_traj']).cpu().numpy()) <= 1e-13
    # a second rollout between forward and backward
    X, U = mpc_rollout_tv(C4, t(C1.x0), K, tAt, None, hold)
    C4.rollout(2)
    with pytest.raises(RuntimeError, match='rolled out again'):
        X.sum().backward()
    with pytest.raises(ValueError):
        mpc_rollout_tv(C4, t(C1.x0), K, None, None, hold)


def test_mpc_rollout_tv_on_the_controllers_stream_makes_no_host_round_trip():
    """Every pointer of the two library calls is a device pointer: forward and backward are stream-ordered on torch's stream."""
    import torch
    from pympc_amd.torch_layer import mpc_rollout_tv
    name, hold = rc.FIRST, 2
    K = rc.CASES[name]['K']
    Adt, Bdt = tc.batch_schedule(name, hold)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        C1 = _ctrl(name, over=dict(stream=stream.cuda_stream))
        dev = torch.device('cuda:0')
        tx = torch.tensor(C1.x0, dtype=torch.float64, device=dev, requires_grad=True)
        tA = torch.tensor(Adt, dtype=torch.float64, device=dev, requires_grad=True)
        tB = torch.tensor(Bdt, dtype=torch.float64, device=dev)
        seen = []
        orig = C1.prob.rollout_adjoint

        def spy(**kw):
            seen.append(all(v is None or (hasattr(v, 'is_cuda') and v.is_cuda) for v in (kw.get('g_x'), kw.get('g_u'))))
            res = orig(**kw)
            seen.append(all(v.is_cuda for v in res.values()))
            return res
        C1.prob.rollout_adjoint = spy
        X, U = mpc_rollout_tv(C1, tx, K, tA, tB, hold)
        assert 'Ad' in C1._on_device and 'Ad' not in C1.__dict__      # (the last entry stays on the device until somebody reads the attribute)
        (X[-1] ** 2).sum().backward()
        assert seen == [True, True] and tx.grad.is_cuda and tA.grad.is_cuda and tuple(tA.grad.shape) == Adt.shape
    stream.synchronize()
    C2 = _ctrl(name)
    C2.update(C1.x0)
    t2 = C2.rollout_tv(K, (Adt, Bdt, hold))
    gx = np.zeros_like(t2['x']); gx[-1] = 2 * t2['x'][-1]
    ref = C2.rollout_adjoint(g_x=gx, want=('lam', 'Ad_traj', 'Ap_traj'))
    assert _rel(tx.grad.cpu().numpy(), ref['lam'][0]) <= 1e-13 and _rel(tA.grad.cpu().numpy(), ref['Ad_traj'] + ref['Ap_traj']) <= 1e-13
    assert np.array_equal(C1.Ad, Adt[-1])


# ---- 9. the constant path did not move -----------------------------------------------------------------------------------------------------
def test_the_unscheduled_sweep_has_the_bits_it_had():
    """rollout_adjoint on case 'first' (every gradient it has, the bounds included) against the bits recorded with the library before the
    schedule (scripts/record_rollout_const_bits.py, tests/golden/rollout_const_bits.npz)."""
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import record_rollout_const_bits as rec
    finally:
        sys.path.pop(0)
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'rollout_const_bits.npz'))
    got = rec.outputs()
    assert sorted(gold.files) == sorted(got)
    for k in gold.files:
        assert got[k].dtype == gold[k].dtype and np.array_equal(got[k], gold[k]), k


# ---- 10. the example -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_learn_plant_parameter_example_recovers_it():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'learn_plant_parameter_through_ltv_mpc.py'), '--batch', '16', '--steps', '12', '--iters', '8'],
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout)
    loss = [float(v) for v in re.findall(r'^iteration +\d+: loss ([0-9.e+-]+)', r.stdout, flags=re.M)]
    assert len(loss) >= 3 and loss[-1] < 1e-2 * loss[0], loss
    m = re.search(r'^parameter: true ([0-9.e+-]+) start ([0-9.e+-]+) learned ([0-9.e+-]+)', r.stdout, flags=re.M)
    true, start, learned = (float(v) for v in m.groups())
    assert abs(learned - true) <= 0.1 * abs(start - true), (true, start, learned)
