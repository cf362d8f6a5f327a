"""The taped rollout with an affine term in the prediction model and its reverse sweep on the device (include_ext5/mpcqp_rollout_affine.h,
pympc_amd/csrc/mpcqp_rollout.h: the affine runtime path of k_rollout_adjoint / k_rollout_adjoint_tv) on the closed loops of
tests/rollout_affine_cases.py: the trajectories and the handle against run(d_traj=, d_hold=), bit for bit; the tape and the term slots against a
twin stepped on the host; the sweep against the numpy restatement tests/rollout_affine_ref.py evaluated on the device's own tape; identities;
determinism; central differences of run(d_traj=) itself; torch; the refusals.

Everything is solved at the project's parity setting eps_abs = eps_rel = 1e-9.  TOL and FD_TOL are those of tests/rollout_dev.py."""
import ctypes as C

import numpy as np
import pytest

import bounds_ref
import rollout_affine_cases as ac
import rollout_affine_ref as ar
import rollout_cases as rc
import rollout_ref as rr
import rollout_tv_cases as tc
from rollout_dev import TOL, FD_TOL, SOLVED, ctrl as _ctrl_of, inputs as _inputs
from util import rel1_any as _rel

pytestmark = pytest.mark.gpu

WEIGHTS = ar.WEIGHT_NAMES
BOUNDS = bounds_ref.NAMES
BASE = ('lam', 'uminus1', 'uref', 'xref')
TRAJ = ('Ad_traj', 'Bd_traj', 'Ap_traj', 'Bp_traj')
TERMS = ('d0', 'd_traj')
PLAIN = BASE + ('Ad', 'Bd', 'Ap', 'Bp') + WEIGHTS + BOUNDS
MODEL_HOLD = 2             # the model schedule of the scheduled variants (tests/rollout_tv_cases.py's, at this hold)
SAME_LOOP = dict(scaling=0, warm_start=0, adaptive_rho=0)      # (tests/test_gpu_rollout_tv.py: settings under which two forms of one loop are the same loop)


def _ctrl(name, seeds=None, **kw):
    return _ctrl_of(name, seeds=ac.SEEDS[name] if seeds is None else seeds, **kw)


def _io(name, own_plant):
    io = _inputs(name, own_plant, own_plant, seeds=ac.SEEDS[name])
    return {k: io[k] for k in ('Ap', 'Bp', 'w')}


def _sched(name, sched):
    return tc.batch_schedule(name, MODEL_HOLD, seeds=ac.SEEDS[name]) + (MODEL_HOLD,) if sched else None


def _begin(Kb, d0):
    """The first solve under d0 (tape entry 0): set_affine and a solve, as update(x, d=) does."""
    Kb.update(Kb.x0, d=d0)
    return Kb


_fwd = {}


def _forward(name, rows, hold, sched=False, own_plant=False):
    """One forward variant made once: rollout_affine(K) on one controller, its tape and its slots.  Nobody changes it."""
    key = (name, rows, hold, sched, own_plant)
    if key not in _fwd:
        K = rc.CASES[name]['K']
        io = _io(name, own_plant)
        d0, dt = ac.batch_terms(name, rows, hold)
        Kb = _begin(_ctrl(name), d0)
        res = Kb.rollout_affine(K, d_traj=dt, d_hold=hold, model_traj=_sched(name, sched), **io)
        _fwd[key] = dict(Kb=Kb, tr=res, io=io, d0=d0, dt=dt, tape=[Kb.prob.rollout_tape(k) for k in range(K)],
                         dslots=[Kb.prob.rollout_affine_slot(s) for s in range(ac.nent(name, hold) + 1)],
                         mslots=[Kb.prob.rollout_tv_slot(s) for s in range(tc.nseg(name, MODEL_HOLD) + 1)] if sched else None,
                         scaling=Kb.prob.scaling()[:3], fresh=None)
    return _fwd[key]


def _seeds(name, B=None):
    c = rc.CASES[name]
    B = len(ac.SEEDS[name]) if B is None else B
    rng = np.random.default_rng(31)
    return rng.standard_normal((c['K'] + 1, B, c['nx'])), rng.standard_normal((c['K'], B, c['nu']))


# ---- 1. forward against the loop ------------------------------------------------------------------------------------------------------------
VARIANTS = [(name, rows, hold, sched) for name in ac.NAMES for rows, hold in ac.combos() for sched in (False, True) if not sched or name in ac.SCHEDULED]


@pytest.mark.parametrize('name,rows,hold,sched', VARIANTS)
def test_rollout_affine_is_run_with_the_schedule(name, rows, hold, sched):
    K = rc.CASES[name]['K']
    for own_plant in (False, True):
        f = _forward(name, rows, hold, sched, own_plant)
        Kb, got, io = f['Kb'], f['tr'], f['io']
        Kd = _begin(_ctrl(name), f['d0'])
        want = Kd.run(K, d_traj=f['dt'], d_hold=hold, model_traj=_sched(name, sched), **io)
        for k in ('x', 'u', 'status', 'iter'):
            assert np.array_equal(got[k], want[k]), (name, rows, hold, k)
        assert np.all(got['status'] == SOLVED)
        for va, vb in zip(Kb.prob.iterate_state(), Kd.prob.iterate_state()):
            assert np.array_equal(va, vb), (name, rows, hold)
        (xa, ya, ia), (xb, yb, ib) = Kb.prob.solution(), Kd.prob.solution()
        assert np.array_equal(xa, xb) and np.array_equal(ya, yb) and [bytes(i) for i in ia] == [bytes(i) for i in ib], (name, rows, hold)
        last = f['dt'][(K - 1) // hold]                    # the controller is left holding the last entry used
        assert np.array_equal(Kb.affine(), last) and np.array_equal(Kd.affine(), last)
        assert np.array_equal(Kb.uminus1_rh, Kd.uminus1_rh) and np.array_equal(Kb.x0_rh, Kd.x0_rh)
        if sched:
            assert np.array_equal(Kb.Ad, Kd.Ad) and np.array_equal(Kb.Bd, Kd.Bd)


# ---- 2. the tape and the slots against the host ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,hold', ac.combos())
@pytest.mark.parametrize('name', ('first', 'hard'))
def test_the_tape_and_the_slots_are_what_the_handle_held(name, rows, hold):
    nx, nu, K = rc.CASES[name]['nx'], rc.CASES[name]['nu'], rc.CASES[name]['K']
    f = _forward(name, rows, hold)
    d0, dt = f['d0'], f['dt']
    want_slots = [d0] + [dt[e] for e in range(dt.shape[0])]
    assert len(f['dslots']) == len(want_slots)
    for s, (a, b) in enumerate(zip(f['dslots'], want_slots)):
        assert np.array_equal(a, b), (name, s)
    for k in range(K):                                     # entry k's step data carry the term of slot tau(k)
        assert np.array_equal(f['tape'][k]['d'], want_slots[ar.tau(k, hold)]), (name, k)
    # the twin: what the handle held before each step, with set_affine(entry); run(1) per step
    Ka = _begin(_ctrl(name), d0)
    um1, xref = np.array(Ka.uminus1), np.array(Ka.xref).reshape(Ka.B, -1)
    for k in range(K):
        x, z, y = Ka.prob.iterate_state()
        status = np.array([i.status for i in Ka.prob.infos()])
        held_d = Ka.affine()
        Ka.set_affine(dt[k // hold])
        t = Ka.run(1)
        e = f['tape'][k]
        for v, h in (('x', x), ('z', z), ('y', y), ('status', status)):
            assert np.array_equal(e[v], h), (name, rows, hold, k, v)
        assert np.array_equal(e['step'][:, :nx], t['x'][0]) and np.array_equal(e['step'][:, nx:nx + nu], um1) and np.array_equal(e['step'][:, nx + nu:], xref)
        assert np.array_equal(e['d'], held_d), (name, k)
        for v in ('x', 'u', 'status', 'iter'):
            assert np.array_equal(f['tr'][v][k + (v == 'x')], t[v][int(v == 'x')]), (name, rows, hold, k, v)
        um1 = t['u'][0].copy()
    bp = f['Kb'].prob
    nr = ac.nrows(name, rows)
    assert bp.rollout_affine_tape_bytes(K, nr, d_hold=hold) > bp.rollout_tape_bytes(K) > 0
    assert bp.rollout_affine_tape_bytes(K, nr, d_hold=hold, model_hold=2) > bp.rollout_tv_tape_bytes(K, 2)
    with pytest.raises(RuntimeError, match=r'\(-1\)'):
        bp.rollout_affine_slot(len(want_slots))


def test_slot_zero_of_a_handle_without_a_term_is_zeros():
    """... written by the call, into entry 0's step data too: a term set and cleared before leaves its doubles in the handle's step blob."""
    name, rows, hold = 'first', 'Np', 1
    K = rc.CASES[name]['K']
    d0, dt = ac.batch_terms(name, rows, hold)
    Kb = _ctrl(name)
    Kb.set_affine(d0 + 1.0)
    Kb.set_affine(None)
    Kb.solve()
    Kb.rollout_affine(K, d_traj=dt, d_hold=hold)
    assert not Kb.prob.rollout_affine_slot(0).any() and not Kb.prob.rollout_tape(0)['d'].any()
    assert np.array_equal(Kb.prob.rollout_tape(1)['d'], dt[0])
    Kc = _ctrl(name)                                       # the same loop on a handle that never had one
    Kc.solve()
    Kc.rollout_affine(K, d_traj=dt, d_hold=hold)
    gx, gu = _seeds(name)
    a, b = Kb.rollout_adjoint(g_x=gx, g_u=gu, want=BASE + TERMS), Kc.rollout_adjoint(g_x=gx, g_u=gu, want=BASE + TERMS)
    for k in BASE + TERMS:
        assert np.array_equal(a[k], b[k]), k


# ---- 3. the reverse sweep against the restatement -------------------------------------------------------------------------------------------
_maps = {}


def _reference(f, name, rows, hold, sched, b, gx, gu):
    """The restatement's sweep of instance b on the device's tape and slots."""
    seed = ac.SEEDS[name][b]
    kw, attrs = rc.draw(name, seed)
    nx, nu = rc.CASES[name]['nx'], rc.CASES[name]['nu']
    tape = [dict(x=e['x'][b], z=e['z'][b], y=e['y'][b], x0=e['step'][b, :nx], um1=e['step'][b, nx:nx + nu], xref=e['step'][b, nx + nu:],
                 solved=bool(e['status'][b] == SOLVED)) for e in f['tape']]
    if sched:
        mslots = []
        for s in f['mslots']:
            blob = s['model']
            mslots.append(dict(Ad=blob[b, :nx * nx].reshape(nx, nx), Bd=blob[b, nx * nx:nx * nx + nx * nu].reshape(nx, nu), D=s['D'][b], E=s['E'][b], c=s['c'][b]))
    else:
        D, E, c = f['scaling']
        mslots = [dict(Ad=np.asarray(kw['Ad'], dtype=float), Bd=np.asarray(kw['Bd'], dtype=float), D=D[b], E=E[b], c=c[b])]
    key = (name, seed, sched)
    if key not in _maps:
        _maps[key] = (bounds_ref.bound_maps(rr.entry_kwargs(kw, tape[0]), attrs), {})
    bmaps, maps = _maps[key]
    io = f['io']
    dsl = np.stack([s[b] for s in f['dslots']])
    return ar.sweep(kw, attrs, tape, dsl, hold, mslots, MODEL_HOLD if sched else 0, gx[:, b], gu[:, b],
                    Ap=None if io['Ap'] is None else io['Ap'][b], Bp=None if io['Bp'] is None else io['Bp'][b], bmaps=bmaps, maps=maps)


@pytest.mark.parametrize('name,rows,hold,sched', VARIANTS)
def test_the_sweep_is_the_restatement(name, rows, hold, sched):
    K, nx = rc.CASES[name]['K'], rc.CASES[name]['nx']
    gx, gu = _seeds(name)
    for own_plant in (False, True):
        f = _forward(name, rows, hold, sched, own_plant)
        Kb = f['Kb']
        names = (BASE + TRAJ + ('Ad', 'Bd', 'Ap', 'Bp') + WEIGHTS + BOUNDS if sched else PLAIN) + TERMS
        got = Kb.rollout_adjoint(g_x=gx, g_u=gu, want=names)
        nact, nweak, status, nfac = Kb.prob.rollout_info()
        assert np.all(status == 1) and np.all(nweak == 0), (name, status, nweak)
        nent, nr = ac.nent(name, hold), ac.nrows(name, rows)
        assert got['d0'].shape == (Kb.B, nr * nx) and got['d_traj'].shape == (nent, Kb.B, nr * nx)
        errs = {}
        for b in range(Kb.B):
            ref = _reference(f, name, rows, hold, sched, b, gx, gu)
            assert np.array_equal(nact[:, b], ref['n_active']) and np.array_equal(nweak[:, b], ref['n_weak']), (name, b, nact[:, b], ref['n_active'])
            assert nfac[b] == ref['n_factor'], (name, rows, hold, b, nfac[b], ref['n_factor'])
            pairs = [(k, got[k][:, b] if k in ('lam', 'xref') else got[k][b], ref[k]) for k in BASE + WEIGHTS + BOUNDS]
            pairs += [('d0', got['d0'][b], ref['d_slots'][0].ravel()), ('d_traj', got['d_traj'][:, b], ref['d_slots'][1:].reshape(nent, -1))]
            if sched:
                pairs += [('Ad_traj', got['Ad_traj'][:, b], ref['Ad_slots'][1:]), ('Bd_traj', got['Bd_traj'][:, b], ref['Bd_slots'][1:]),
                          ('Ap_traj', got['Ap_traj'][:, b], ref['Ap_entries']), ('Bp_traj', got['Bp_traj'][:, b], ref['Bp_entries']),
                          ('Ad', got['Ad'][b], ref['Ad_slots'][0]), ('Bd', got['Bd'][b], ref['Bd_slots'][0])]
            else:
                pairs += [('Ad', got['Ad'][b], ref['Ad_slots'][0]), ('Bd', got['Bd'][b], ref['Bd_slots'][0]),
                          ('Ap', got['Ap'][b], ref['Ap_entries'][0]), ('Bp', got['Bp'][b], ref['Bp_entries'][0])]
            for k, v, r in pairs:
                errs[k] = max(errs.get(k, 0.0), _rel(v, r))
            for e in range(nent):                          # a slot no tape entry used is exactly zero
                if not any(ar.tau(k, hold) == e + 1 for k in range(K)):
                    assert not got['d_traj'][e, b].any(), (name, e)
            assert got['d_traj'][0, b].any() and got['d0'][b].any()
        worst = max(errs.values())
        print('ROLLOUT_AFFINE_ERR %s rows %s hold %d %s plant %s: max %.3e  %s' % (name, rows, hold, 'sched' if sched else 'model', 'given' if own_plant else 'follows', worst,
                                                                               ' '.join('%s=%.1e' % kv for kv in errs.items())))
        assert worst <= TOL, (name, rows, hold, errs)


# ---- 4. identities at 1e-13 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', ac.ROWS)
def test_a_schedule_of_the_constant_term_sums_to_the_constant_tape(rows):
    name, hold = 'first', 2
    K = rc.CASES[name]['K']
    d0, _ = ac.batch_terms(name, rows, hold)
    dt = np.repeat(d0[None], ac.nent(name, hold), axis=0)
    Ks, Kc = _begin(_ctrl(name, **SAME_LOOP), d0), _begin(_ctrl(name, **SAME_LOOP), d0)
    ts, tcn = Ks.rollout_affine(K, d_traj=dt, d_hold=hold), Kc.rollout_affine(K)
    for k in ('x', 'u', 'status', 'iter'):
        assert np.array_equal(ts[k], tcn[k]), k
    gx, gu = _seeds(name)
    got, ref = Ks.rollout_adjoint(g_x=gx, g_u=gu, want=PLAIN + TERMS), Kc.rollout_adjoint(g_x=gx, g_u=gu, want=PLAIN + ('d0',))
    assert np.all(got['status'] == 1) and np.all(ref['status'] == 1)
    errs = {k: _rel(got[k], ref[k]) for k in PLAIN}
    errs['d'] = _rel(got['d0'] + got['d_traj'].sum(axis=0), ref['d0'])
    print('ROLLOUT_AFFINE_CONST rows %s: %s' % (rows, ' '.join('%s=%.1e' % kv for kv in errs.items())))
    assert max(errs.values()) <= 1e-13, errs
    with pytest.raises(RuntimeError, match='d_traj'):      # a tape of one constant term has no schedule to differentiate
        Kc.rollout_adjoint(g_x=gx, g_u=gu, want=('d_traj',))


def test_a_one_row_term_is_the_stage_sum_of_the_same_row_repeated():
    name, hold = 'first', 2
    c = rc.CASES[name]
    K, Np, nx = c['K'], c['Np'], c['nx']
    d0, dt = ac.batch_terms(name, '1', hold)               # [B, 1, nx], [nent, B, 1, nx]
    K1, KN = _begin(_ctrl(name), d0), _begin(_ctrl(name), np.repeat(d0, Np, axis=1))
    t1, tN = K1.rollout_affine(K, d_traj=dt, d_hold=hold), KN.rollout_affine(K, d_traj=np.repeat(dt, Np, axis=2), d_hold=hold)
    for k in ('x', 'u', 'status', 'iter'):
        assert np.array_equal(t1[k], tN[k]), k
    gx, gu = _seeds(name)
    a, b = K1.rollout_adjoint(g_x=gx, g_u=gu, want=TERMS), KN.rollout_adjoint(g_x=gx, g_u=gu, want=TERMS)
    B = K1.B
    assert _rel(a['d0'], b['d0'].reshape(B, Np, nx).sum(axis=1)) <= 1e-13
    assert _rel(a['d_traj'], b['d_traj'].reshape(-1, B, Np, nx).sum(axis=2)) <= 1e-13


@pytest.mark.parametrize('rows', ac.ROWS)
def test_one_step_is_the_adjoint_of_that_solve(rows):
    name = 'held'
    d0, dt = ac.batch_terms(name, rows, 1)
    Kb = _begin(_ctrl(name), d0)
    gu = _seeds(name)[1][:1]
    one = Kb.adjoint(g_u0=gu[0], want=('d', 'x0'))
    Kb.rollout_affine(1, d_traj=dt[:1], d_hold=1)
    got = Kb.rollout_adjoint(g_u=gu, want=('d0', 'd_traj', 'lam'))
    assert _rel(got['d0'], one['d']) <= 1e-13 and _rel(got['lam'][0], one['x0']) <= 1e-13
    assert not got['d_traj'].any()                         # (entry 0's only solve is the one for x_1, which is on no tape)


def test_a_schedule_of_zeros_on_a_handle_without_a_term_is_the_plain_rollout():
    name, hold = 'first', 1
    c = rc.CASES[name]
    K = c['K']
    io = _io(name, True)
    Ka, Kp = _ctrl(name), _ctrl(name)
    ta = Ka.rollout_affine(K, d_traj=np.zeros((K, Ka.B, c['nx'])), d_hold=hold, **io)
    tp = Kp.rollout(K, **io)
    for k in ('x', 'u', 'status', 'iter'):
        assert np.array_equal(ta[k], tp[k]), k
    gx, gu = _seeds(name)
    a, p = Ka.rollout_adjoint(g_x=gx, g_u=gu, want=PLAIN + TERMS), Kp.rollout_adjoint(g_x=gx, g_u=gu, want=PLAIN)
    for k in PLAIN + ('n_factor', 'status', 'n_weak'):
        assert np.array_equal(a[k], p[k]), k
    assert a['d_traj'].any()


# ---- 5. determinism --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sched', (False, True), ids=('one_model', 'model_schedule'))
def test_two_sweeps_reuse_alone_and_batch_sum(sched):
    name, rows, hold = 'first', 'Np', 2
    f = _forward(name, rows, hold, sched)
    Kb, K = f['Kb'], rc.CASES[name]['K']
    gx, gu = _seeds(name)
    names = (BASE + TRAJ + WEIGHTS + BOUNDS if sched else PLAIN) + TERMS
    a, b = Kb.rollout_adjoint(g_x=gx, g_u=gu, want=names), Kb.rollout_adjoint(g_x=gx, g_u=gu, want=names)
    for k in names + ('n_factor',):
        assert np.array_equal(a[k], b[k]), k
    nr = Kb.rollout_adjoint(g_x=gx, g_u=gu, want=names, no_reuse=True)
    for k in names:
        assert np.array_equal(a[k], nr[k]), k
    assert np.all(nr['n_factor'] == K) and (sched or np.any(a['n_factor'] < K))
    alone = Kb.rollout_adjoint(g_x=gx, g_u=gu, want=('d_traj',))
    assert np.array_equal(alone['d_traj'], a['d_traj'])
    s = Kb.rollout_adjoint(g_x=gx, g_u=gu, want=TERMS + ('Qx',), batch_sum=True)
    assert s['d_traj'].shape == (a['d_traj'].shape[0], 1, a['d_traj'].shape[2]) and s['d0'].shape == (1, a['d0'].shape[1])
    assert _rel(s['d_traj'], a['d_traj'].sum(axis=1, keepdims=True)) <= 1e-13 and _rel(s['d0'], a['d0'].sum(axis=0, keepdims=True)) <= 1e-13


# ---- 6. end to end: central differences of run(d_traj=) itself -------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', ac.ROWS)
def test_the_sweep_against_central_differences_of_the_device_loop(rows):
    """L = sum <Gx[k], x_k> + sum <Gu[k], u_k> of run(K, d_traj=, d_hold=2) on fresh controllers, in a direction of x0, one of d0 and one of the
    whole schedule, each normalised per instance."""
    name, hold = 'first', 2
    K, B = rc.CASES[name]['K'], len(ac.SEEDS[name])
    gx, gu = _seeds(name)
    f = _forward(name, rows, hold)
    got = f['Kb'].rollout_adjoint(g_x=gx, g_u=gu, want=('lam',) + TERMS)
    assert np.all(got['status'] == 1) and np.all(got['n_weak'] == 0)
    d0, dt = f['d0'], f['dt']
    base = rc.batch_kwargs(name, ac.SEEDS[name])
    rng = np.random.default_rng(37)
    h = 1e-4

    def loss(x0, a0, at):
        Kf = _ctrl(name, over=dict(x0=x0))
        Kf.update(x0, d=a0)
        t = Kf.run(K, d_traj=at, d_hold=hold)
        return (gx * t['x']).sum(axis=(0, 2)) + (gu * t['u']).sum(axis=(0, 2))      # per instance: they are independent

    def unit(shape, axis_b):
        d = rng.standard_normal(shape)
        n = np.sqrt((np.moveaxis(d, axis_b, 0).reshape(B, -1) ** 2).sum(axis=1))
        return d / n.reshape([B if i == axis_b else 1 for i in range(d.ndim)])

    v = unit(base['x0'].shape, 0)
    checks = [('x0', (got['lam'][0] * v).sum(axis=1), (loss(base['x0'] + h * v, d0, dt) - loss(base['x0'] - h * v, d0, dt)) / (2 * h))]
    v = unit(d0.shape, 0)
    checks.append(('d0', (got['d0'] * v.reshape(B, -1)).sum(axis=1), (loss(base['x0'], d0 + h * v, dt) - loss(base['x0'], d0 - h * v, dt)) / (2 * h)))
    v = unit(dt.shape, 1)
    checks.append(('d_traj', (got['d_traj'] * v.reshape(dt.shape[0], B, -1)).sum(axis=(0, 2)), (loss(base['x0'], d0, dt + h * v) - loss(base['x0'], d0, dt - h * v)) / (2 * h)))
    for field, an, fd in checks:
        err = np.abs(an - fd).max()
        print('ROLLOUT_AFFINE_FD rows %s d/d%s: |grad.d - FD|_inf = %.3e, |FD|_inf = %.3e' % (rows, field, err, np.abs(fd).max()))
        assert err <= FD_TOL * max(1.0, np.abs(fd).max()), (field, err, an, fd)
        assert np.abs(fd).max() > 1e-2


# ---- 7. K_d ----------------------------------------------------------------------------------------------------------------------------------
def _kd_ctrl(name, rows):
    """(controller of the case with a term in force and solved, the term [B, rows, nx]); nb64 is a case of tests/rollout_cases.py, no loop needed."""
    seeds = ac.SEEDS[name] if name in ac.SEEDS else rc.CASES[name]['seeds']
    c = rc.CASES[name]
    Kb = _ctrl_of(name, seeds=seeds)
    s = ac.SCALE * np.maximum(1.0, np.abs(Kb.x0).max(axis=1))
    d = s[:, None, None] * np.random.default_rng(7).standard_normal((Kb.B, c['Np'] if rows == 'Np' else 1, c['nx']))
    Kb.update(Kb.x0, d=d)
    return Kb, d


@pytest.mark.parametrize('rows', ac.ROWS)
@pytest.mark.parametrize('name', ('held', 'nb64'))
def test_every_row_of_K_d_is_the_adjoint_of_its_unit_seed(name, rows):
    """held: NB <= 32 and nu = 3, no multiple of four (seeds four to a solve, one column idle); nb64: seeds one to a solve."""
    Kb, d = _kd_ctrl(name, rows)
    g = Kb.gains()
    nu, w = Kb.nu, d.shape[1] * Kb.nx
    assert g['K_d'].shape == (Kb.B, nu, w) and np.all(g['status'] == 1)
    plain = {k: g[k].copy() for k in ('K_x0', 'K_um1', 'K_xref', 'K_uref')}
    for j in range(nu):
        e = np.zeros((Kb.B, nu)); e[:, j] = 1.0
        one = Kb.adjoint(g_u0=e, want=('d', 'x0'))
        assert _rel(g['K_d'][:, j], one['d']) <= 1e-13, (name, rows, j, _rel(g['K_d'][:, j], one['d']))
        assert _rel(g['K_x0'][:, j], one['x0']) <= 1e-13
    assert np.abs(g['K_d']).max() > 1e-3
    from pympc_amd import _lib                               # the other four gains are those of mpcqp_gains itself, bit for bit
    old = [np.empty_like(plain[k]) for k in ('K_x0', 'K_um1', 'K_xref', 'K_uref')]
    assert Kb.prob._L.mpcqp_gains(Kb.prob._h, *[C.c_void_p(a.ctypes.data) for a in old]) == 0
    for a, k in zip(old, ('K_x0', 'K_um1', 'K_xref', 'K_uref')):
        assert np.array_equal(a, plain[k]), k


@pytest.mark.parametrize('rows', ac.ROWS)
def test_K_d_against_central_differences_of_the_step(rows):
    name = 'held'
    Kb, d = _kd_ctrl(name, rows)
    g = Kb.gains()
    assert np.all(g['n_weak'] == 0)
    x0, um1 = Kb.x0.copy(), np.array(Kb.uminus1)
    rng = np.random.default_rng(41)
    v = rng.standard_normal(d.shape)
    v /= np.sqrt((v.reshape(Kb.B, -1) ** 2).sum(axis=1))[:, None, None]
    h = 1e-4
    up = np.array(_ctrl_of(name, seeds=ac.SEEDS[name]).step(x0, um1, d=d + h * v))
    dn = np.array(_ctrl_of(name, seeds=ac.SEEDS[name]).step(x0, um1, d=d - h * v))
    fd = (up - dn) / (2 * h)
    an = np.einsum('bjw,bw->bj', g['K_d'], v.reshape(Kb.B, -1))
    err = np.abs(an - fd).max()
    print('K_D_FD rows %s: |K_d v - FD|_inf = %.3e, |FD|_inf = %.3e' % (rows, err, np.abs(fd).max()))
    assert err <= FD_TOL * max(1.0, np.abs(fd).max()), (err, an, fd)
    assert np.abs(fd).max() > 1e-2


def test_no_K_d_without_a_term():
    Kb = _ctrl('held')
    assert 'K_d' not in Kb.gains()
    from pympc_amd import _lib
    p = np.empty((Kb.B, Kb.nu, Kb.nx))
    assert Kb.prob._L.mpcqp_gains_affine(Kb.prob._h, C.c_void_p(p.ctypes.data), None, None, None, C.c_void_p(p.ctypes.data)) == -5
    Kb.update(Kb.x0, d=np.zeros((Kb.B, Kb.nx)))
    assert 'K_d' in Kb.gains()
    Kb.set_affine(None); Kb.solve()
    assert set(Kb.gains()) == {'K_x0', 'K_um1', 'K_xref', 'K_uref', 'n_weak', 'status'}


# ---- 8. torch --------------------------------------------------------------------------------------------------------------------------------
def test_mpc_rollout_affine_is_one_sweep_with_the_matching_seeds():
    import torch
    from pympc_amd.torch_layer import mpc_rollout_affine
    name, hold = 'first', 2
    c = rc.CASES[name]
    K, nx, nu = c['K'], c['nx'], c['nu']
    Adt, Bdt, mh = _sched(name, True)
    d0, dt = ac.batch_terms(name, '1', hold)               # [B, 1, nx], [nent, B, 1, nx]
    dev = torch.device('cuda:0')
    t = lambda a, g=True: torch.tensor(np.asarray(a, dtype=float), dtype=torch.float64, device=dev, requires_grad=g)
    wx, wu = torch.tensor(_seeds(name)[0], device=dev), torch.tensor(_seeds(name)[1], device=dev)
    loss_of = lambda X, U: 0.5 * (wx * X * X).sum() + 0.5 * (wu * U * U).sum()
    C1 = _ctrl(name)
    B = C1.B
    tx, td0, td, tAt, tBt = t(C1.x0), t(d0[:, 0]), t(dt[:, :, 0]), t(Adt), t(Bdt)
    X, U = mpc_rollout_affine(C1, tx, K, td, d_hold=hold, d0=td0, Ad_traj=tAt, Bd_traj=tBt, hold=mh)
    assert X.shape == (K + 1, B, nx) and U.shape == (K, B, nu) and X.is_cuda
    grads = torch.autograd.grad(loss_of(X, U), [tx, td0, td, tAt])
    assert np.array_equal(C1.affine(), dt[-1])
    C2 = _begin(_ctrl(name), d0)
    ref_tr = C2.rollout_affine(K, d_traj=dt, d_hold=hold, model_traj=(Adt, Bdt, mh))
    assert np.array_equal(X.detach().cpu().numpy(), ref_tr['x']) and np.array_equal(U.detach().cpu().numpy(), ref_tr['u'])
    gx, gu = wx.cpu().numpy() * ref_tr['x'], wu.cpu().numpy() * ref_tr['u']
    ref = C2.rollout_adjoint(g_x=gx, g_u=gu, want=('lam', 'd0', 'd_traj', 'Ad_traj', 'Ap_traj'))
    want = [ref['lam'][0], ref['d0'], ref['d_traj'], ref['Ad_traj'] + ref['Ap_traj']]
    for g, w_, n in zip(grads, want, ('x0', 'd0', 'd', 'Ad_traj')):
        assert tuple(g.shape) == tuple(np.shape(w_)) and g.is_cuda, n
        assert _rel(g.cpu().numpy(), w_) <= 1e-13, (n, _rel(g.cpu().numpy(), w_))
    # the plant carries the offset too: its gradient arrives through w, entry e gets lam[k + 1] of the steps it was in force
    C3 = _ctrl(name)
    td = t(dt[:, :, 0])
    X, U = mpc_rollout_affine(C3, t(C1.x0, False), K, td, d_hold=hold, d0=t(d0[:, 0], False), offset_in_plant=True)
    gd, = torch.autograd.grad(loss_of(X, U), [td])
    r3 = C3.prob.rollout_adjoint(g_x=(wx * X).detach(), g_u=(wu * U).detach(), want=('lam', 'd_traj'))
    lam = r3['lam'].cpu().numpy()
    through_w = np.stack([lam[1 + e * hold:1 + min((e + 1) * hold, K)].sum(axis=0) for e in range(dt.shape[0])])
    assert _rel(gd.cpu().numpy(), r3['d_traj'].cpu().numpy() + through_w) <= 1e-13
    C4 = _ctrl(name)                                       # ... which is run(d_traj=) with the offset in w
    C4.update(C4.x0, d=d0)
    t4 = C4.run(K, d_traj=dt, d_hold=hold, w=np.repeat(dt[:, :, 0], hold, axis=0)[:K])
    assert np.array_equal(X.detach().cpu().numpy(), t4['x'])
    with pytest.raises(ValueError, match='one-row'):
        mpc_rollout_affine(C4, t(C1.x0), K, t(ac.batch_terms(name, 'Np', hold)[1]), d_hold=hold, offset_in_plant=True)
    # a second rollout between forward and backward
    X, U = mpc_rollout_affine(C4, t(C1.x0), K, t(dt[:, :, 0]), d_hold=hold)
    C4.rollout_affine(2)
    with pytest.raises(RuntimeError, match='rolled out again'):
        X.sum().backward()


def test_mpc_rollout_affine_on_the_controllers_stream_makes_no_host_round_trip():
    """Every pointer of the two library calls is a device pointer: forward and backward are stream-ordered on torch's stream."""
    import torch
    from pympc_amd.torch_layer import mpc_rollout_affine
    name, hold = 'first', 2
    K = rc.CASES[name]['K']
    d0, dt = ac.batch_terms(name, 'Np', hold)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        C1 = _ctrl(name, over=dict(stream=stream.cuda_stream))
        dev = torch.device('cuda:0')
        tx = torch.tensor(C1.x0, dtype=torch.float64, device=dev, requires_grad=True)
        td = torch.tensor(dt, dtype=torch.float64, device=dev, requires_grad=True)
        td0 = torch.tensor(d0, dtype=torch.float64, device=dev, requires_grad=True)
        seen = []
        orig = C1.prob.rollout_adjoint

        def spy(**kw):
            seen.append(all(v is None or (hasattr(v, 'is_cuda') and v.is_cuda) for v in (kw.get('g_x'), kw.get('g_u'))))
            res = orig(**kw)
            seen.append(all(v.is_cuda for v in res.values()))
            return res
        C1.prob.rollout_adjoint = spy
        X, U = mpc_rollout_affine(C1, tx, K, td, d_hold=hold, d0=td0)
        (X[-1] ** 2).sum().backward()
        assert seen == [True, True] and tx.grad.is_cuda and td.grad.is_cuda and tuple(td.grad.shape) == dt.shape and tuple(td0.grad.shape) == d0.shape
    stream.synchronize()
    C2 = _begin(_ctrl(name), d0)
    t2 = C2.rollout_affine(K, d_traj=dt, d_hold=hold)
    gx = np.zeros_like(t2['x']); gx[-1] = 2 * t2['x'][-1]
    ref = C2.rollout_adjoint(g_x=gx, want=('lam', 'd0', 'd_traj'))
    assert _rel(tx.grad.cpu().numpy(), ref['lam'][0]) <= 1e-13
    assert _rel(td.grad.cpu().numpy().reshape(ref['d_traj'].shape), ref['d_traj']) <= 1e-13 and _rel(td0.grad.cpu().numpy().reshape(ref['d0'].shape), ref['d0']) <= 1e-13


# ---- 9. the refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_kind_of_the_tape():
    from pympc_amd import _lib
    name = 'first'
    c = rc.CASES[name]
    K, nx, nu, Np = c['K'], c['nx'], c['nu'], c['Np']
    Kt = _ctrl(name)
    bp = Kt.prob
    L, h = bp._L, bp._h
    B = Kt.B
    gx, gu = _seeds(name)
    d0, dt = ac.batch_terms(name, '1', 2)
    dflat = np.ascontiguousarray(dt.reshape(dt.shape[0], B, -1))
    io = _lib.RolloutAdjointIO(); io.struct_size = C.sizeof(_lib.RolloutAdjointIO); io.G_x, io.G_u = gx.ctypes.data, gu.ctypes.data
    at = _lib.AffineTraj(); at.struct_size, at.hold, at.nentries, at.rows, at.d = C.sizeof(_lib.AffineTraj), 2, dflat.shape[0], 1, dflat.ctypes.data
    ao = _lib.RolloutAffineIO(); ao.struct_size = C.sizeof(_lib.RolloutAffineIO)
    state = lambda: tuple(bp.iterate_state()) + (bp.solution()[0],)
    err = lambda: L.mpcqp_last_error().decode()

    def refused(lo, at_struct):
        """mpcqp_rollout_affine's return code; nothing of the iterate or the solution has changed, and nothing was solved."""
        before, count = state(), Kt.solve_count
        code = L.mpcqp_rollout_affine(h, K, C.byref(lo), None, None if at_struct is None else C.byref(at_struct))
        for a, b in zip(before, state()):
            assert np.array_equal(a, b)
        assert Kt.solve_count == count
        return code
    assert refused(_lib.Loop(), None) == -5 and 'mpcqp_set_affine' in err()      # d_traj=None without a handle term
    with pytest.raises(RuntimeError, match='set_affine'):
        Kt.rollout_affine(K)
    for change in (dict(struct_size=8), dict(hold=0), dict(nentries=dflat.shape[0] - 1), dict(rows=2), dict(d=None)):
        bad = _lib.AffineTraj(); C.memmove(C.byref(bad), C.byref(at), C.sizeof(at))
        for k, v in change.items():
            setattr(bad, k, v)
        assert refused(_lib.Loop(), bad) == -1, change
    lo = _lib.Loop(); lo.ny = 1
    assert refused(lo, at) == -4                           # an estimator
    Kt.update(Kt.x0, d=np.repeat(d0, Np, axis=1))          # a handle term of Np rows under a schedule of one
    assert refused(_lib.Loop(), at) == -1 and 'rows' in err()
    count = Kt.solve_count
    with pytest.raises(RuntimeError, match=r'\(-1\)'):
        Kt.rollout_affine(K, d_traj=dt, d_hold=2)
    assert Kt.solve_count == count
    Kt.update(Kt.x0, d=d0)
    bp.update_settings(polish=True)
    assert refused(_lib.Loop(), at) == -4                  # polishing inside the loop
    bp.update_settings(polish=False)
    Kt.update(Kt.x0, solve=False)
    assert refused(_lib.Loop(), at) == -5                  # no solve behind the step data
    Kt.solve()
    n = C.c_int64()
    assert L.mpcqp_rollout_affine_tape_bytes(h, K, 0, 2, 3, C.byref(n)) == -1
    # the order: a mismatch of the rows is said before anything of the schedule's struct, output feedback behind the schedule's own refusals
    Kt.set_affine(np.repeat(d0, Np, axis=1)); Kt.solve()
    bad = _lib.AffineTraj(); C.memmove(C.byref(bad), C.byref(at), C.sizeof(at)); bad.hold = 0
    assert refused(_lib.Loop(), bad) == -1 and 'rows' in err()
    Kt.set_affine(d0); Kt.solve()
    lo = _lib.Loop(); lo.ny = 1
    assert refused(lo, bad) == -1 and 'hold' in err()
    # the kind of the tape: the new sweep on each older kind, the old sweeps on the new kind
    Kt.set_affine(None); Kt.solve()
    Kt.rollout(K)
    assert L.mpcqp_rollout_adjoint_affine(h, C.byref(io), None, None, None, C.byref(ao)) == -5 and 'mpcqp_rollout_affine' in err()
    for names in (('d0',), ('d_traj',)):
        with pytest.raises(RuntimeError, match='rollout_affine'):
            Kt.rollout_adjoint(g_x=gx, g_u=gu, want=names)
    with pytest.raises(RuntimeError, match='rollout_affine'):
        bp.rollout_affine_slot(0)
    Adt, Bdt, mh = _sched(name, True)
    to = _lib.RolloutTVIO(); to.struct_size = C.sizeof(_lib.RolloutTVIO)
    Kt.rollout_tv(K, (Adt, Bdt, mh))
    assert L.mpcqp_rollout_adjoint_affine(h, C.byref(io), None, None, C.byref(to), C.byref(ao)) == -5
    with pytest.raises(RuntimeError, match='rollout_affine'):
        Kt.rollout_adjoint(g_x=gx, g_u=gu, want=('d_traj',))
    # ... the two output-feedback kinds: the tape of a rollout_est and of a rollout_tv_est
    import rollout_est_cases as ec
    from rollout_dev import estimator
    e = ec.batch_estimator(name, ac.SEEDS[name])
    Kt.rollout_est(K, estimator(Kt, e))
    assert L.mpcqp_rollout_adjoint_affine(h, C.byref(io), None, None, None, C.byref(ao)) == -5 and 'not one of mpcqp_rollout_affine' in err()
    with pytest.raises(RuntimeError, match='rollout_affine'):
        Kt.rollout_adjoint(g_x=gx, g_u=gu, want=('d0',))
    Kt.rollout_tv_est(K, (Adt, Bdt, mh), estimator(Kt, e))
    for with_to in (None, C.byref(to)):
        assert L.mpcqp_rollout_adjoint_affine(h, C.byref(io), None, None, with_to, C.byref(ao)) == -5 and 'not one of mpcqp_rollout_affine' in err()
    with pytest.raises(RuntimeError, match='rollout_affine'):
        Kt.rollout_adjoint(g_x=gx, g_u=gu, want=('d_traj',))
    Kt.rollout_affine(K, d_traj=dt, d_hold=2, model_traj=(Adt, Bdt, mh))
    eo = _lib.RolloutEstIO(); eo.struct_size = C.sizeof(_lib.RolloutEstIO)
    bo = _lib.AdjointBoundsIO(); bo.struct_size = C.sizeof(_lib.AdjointBoundsIO)
    xo = _lib.RolloutTVEstIO(); xo.struct_size = C.sizeof(_lib.RolloutTVEstIO)
    lam = np.empty((K + 1, B, nx)); io.lam = lam.ctypes.data
    for code, what in ((L.mpcqp_rollout_adjoint(h, C.byref(io), None), 'mpcqp_rollout_adjoint'),
                       (L.mpcqp_rollout_adjoint_tv_est(h, C.byref(io), C.byref(eo), None, None, C.byref(to), C.byref(xo)), 'mpcqp_rollout_adjoint_tv_est'),
                       (L.mpcqp_rollout_adjoint_est(h, C.byref(io), C.byref(eo), None), 'mpcqp_rollout_adjoint_est'),
                       (L.mpcqp_rollout_adjoint_bounds(h, C.byref(io), None, None, C.byref(bo)), 'mpcqp_rollout_adjoint_bounds'),
                       (L.mpcqp_rollout_adjoint_tv(h, C.byref(io), None, None, C.byref(to)), 'mpcqp_rollout_adjoint_tv')):
        assert code == -5 and 'mpcqp_rollout_adjoint_affine' in err(), what
    assert L.mpcqp_rollout_adjoint_affine(h, C.byref(io), None, None, None, C.byref(ao)) == -5      # a scheduled tape needs its mpcqp_rollout_tv_io
    short = _lib.RolloutAffineIO(); short.struct_size = 8
    assert L.mpcqp_rollout_adjoint_affine(h, C.byref(io), None, None, C.byref(to), C.byref(short)) == -1
    assert L.mpcqp_rollout_adjoint_affine(h, C.byref(io), None, None, C.byref(to), None) == 0        # (every struct but the seeds' and, here, `to` is optional)
    ref = Kt.rollout_adjoint(g_x=gx, g_u=gu, want=BASE + TRAJ + TERMS)
    assert np.array_equal(lam, ref['lam']) and np.all(ref['status'] == 1)
    Kt.rollout_affine(K, d_traj=dt, d_hold=2)              # ... and an unscheduled one must not be given it
    assert L.mpcqp_rollout_adjoint_affine(h, C.byref(io), None, None, C.byref(to), C.byref(ao)) == -5
    # the tape is a copy, its terms included: another term, steps and solves in between change no bit of the sweep
    ref = Kt.rollout_adjoint(g_x=gx, g_u=gu, want=PLAIN + TERMS)
    Kt.step(Kt.x0_rh * 0.9, d=d0 * 0.5)
    again = Kt.rollout_adjoint(g_x=gx, g_u=gu, want=PLAIN + TERMS)
    for k in PLAIN + TERMS + ('n_factor',):
        assert np.array_equal(again[k], ref[k]), k
    # the older calls keep refusing a handle that has a term, and their sweep a tape without one under it
    with pytest.raises(NotImplementedError, match='mpcqp_affine.h'):
        Kt.rollout(K)
    count = Kt.solve_count
    with pytest.raises(NotImplementedError):               # (output feedback with a schedule of terms: refused before the estimator is looked at)
        Kt.run(2, estimator=object(), d_traj=dt, d_hold=2)
    assert Kt.solve_count == count
    bp.rollout_release()
    assert L.mpcqp_rollout_adjoint_affine(h, C.byref(io), None, None, None, C.byref(ao)) == -5


# ---- 10. the example -------------------------------------------------------------------------------------------------------------------------
def test_learn_plant_parameter_affine_example_recovers_it():
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'examples', 'learn_plant_parameter_through_ltv_affine_mpc.py'), '--batch', '16', '--steps', '12', '--iters', '8'],
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout)
    m = re.search(r'^parameter: true ([0-9.e+-]+) start ([0-9.e+-]+) learned ([0-9.e+-]+)', r.stdout, flags=re.M)
    true, start, learned = (float(v) for v in m.groups())
    assert abs(learned - true) <= 0.1 * abs(start - true), (true, start, learned)
