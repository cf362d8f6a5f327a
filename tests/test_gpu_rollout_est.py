"""The taped rollout of the output-feedback loop and its reverse sweep through the estimator on the device (include/mpcqp_rollout_est.h,
pympc_amd/csrc/mpcqp_rollout.h) on the loops of tests/rollout_est_cases.py: the trajectories and the handle against K one-step device
loops with an estimator, bit for bit; the tape against what those loops held between the steps; the sweep against the numpy restatement
tests/rollout_est_ref.py evaluated on the device's own tape and scaling; the factor reuse; K = 1 against mpcqp_adjoint_model; central
differences of run(estimator=...) itself; a failed step; refusals; the state-feedback sweep unmoved; torch; the example.

Everything is solved at the project's parity setting eps_abs = eps_rel = 1e-9.  TOL and FD_TOL are those of tests/test_gpu_rollout.py."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import rollout_cases as rc
import rollout_est_cases as ec
import rollout_est_ref as er
import rollout_dev as rd
from rollout_dev import TOL, FD_TOL, SOLVED, CHAIN, estimator as _estimator
from util import rel1_any as _rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ESTG = ('eta', 'C', 'L', 'v', 'Ae', 'Be')
MODEL = er.MODEL_NAMES
EVERY = CHAIN + ESTG + MODEL
PER_STEP = ('lam', 'eta', 'xref', 'v')                     # [K(+1), B, .]: instance b is [:, b]
NAMES = sorted(ec.SEEDS)
_ctrl, _inputs, _twin, _forward, _ref_tape = (functools.partial(f, est=True) for f in (rd.ctrl, rd.inputs, rd.twin, rd.forward, rd.ref_tape))


def _reference(f, name, b, g):
    """The restatement's sweep of instance b on the device's tape; g = dict(x=, xh=, u=, y=) of [., B, .] seeds or None."""
    kw, attrs = rc.draw(name, f['seeds'][b])
    st = f['refs'].setdefault(b, {})
    tape = _ref_tape(f, name, b)
    if 'maps' not in st:
        st['maps'], st['cache'] = er.adjoint_ref.parameter_maps(er.rollout_ref.entry_kwargs(kw, tape[0]), attrs), {}
    D, E, cs = f['scaling']
    io = f['io']
    pick = lambda a: None if a is None else a[:, b]
    return er.sweep(kw, attrs, tape, D[b], E[b], cs[b], io['e']['C'][b], io['e']['L'][b], G_x=pick(g['x']), G_xh=pick(g['xh']), G_u=pick(g['u']), G_y=pick(g['y']),
                    Ap=None if io['Ap'] is None else io['Ap'][b], Bp=None if io['Bp'] is None else io['Bp'][b], maps=st['maps'], cache=st['cache'])


def _seeds(name, kind, B=None):
    """Seeds of a sweep: kind names them, 'x', 'h' (xhat), 'u', 'y'."""
    c = rc.CASES[name]
    B = len(ec.SEEDS[name]) if B is None else B
    K, nx, nu, ny = c['K'], c['nx'], c['nu'], ec.ny_of(name)
    rng = np.random.default_rng(23)
    g = dict(x=rng.standard_normal((K + 1, B, nx)), xh=rng.standard_normal((K + 1, B, nx)), u=rng.standard_normal((K, B, nu)), y=rng.standard_normal((K, B, ny)))
    return {k: (v if {'x': 'x', 'xh': 'h', 'u': 'u', 'y': 'y'}[k] in kind else None) for k, v in g.items()}


def _sweep(K, g, **kw):
    return K.rollout_adjoint(g_x=g['x'], g_u=g['u'], g_xhat=g['xh'], g_y=g['y'], **kw)


def _compare(f, name, got, g, K):
    """Every output of a sweep against the restatement, every instance; returns the worst relative error by output."""
    nact = K.prob.rollout_info()[0]
    errs = {}
    for b in range(K.B):
        ref = _reference(f, name, b, g)
        assert np.array_equal(nact[:, b], ref['n_active']) and np.array_equal(got['n_weak'][:, b], ref['n_weak']), (name, b, nact[:, b], ref['n_active'])
        assert np.array_equal(got['status'][:, b], ref['status']) and got['n_factor'][b] == ref['n_factor'], (name, b, got['status'][:, b], got['n_factor'][b], ref['n_factor'])
        for k in EVERY:
            v = got[k][:, b] if k in PER_STEP else got[k][b]
            errs[k] = max(errs.get(k, 0.0), _rel(v, ref[k]))
    return errs


# ---- 1. trajectories and the handle afterwards --------------------------------------------------------------------------------------------
def _same_forward(name, tr, seq, Ka, Kb, esta, x_true_b):
    K = rc.CASES[name]['K']
    for k in range(K):
        s = seq[k]
        for v in ('x', 'xhat'):
            assert np.array_equal(tr[v][k], s[v][0]) and np.array_equal(tr[v][k + 1], s[v][1]), (name, k, v)
        for v in ('y', 'u', 'status', 'iter'):
            assert np.array_equal(tr[v][k], s[v][0]), (name, k, v)
    assert np.array_equal(x_true_b, esta.x_true) and np.array_equal(x_true_b, tr['x'][-1]), name
    a, b = Ka.prob, Kb.prob
    for va, vb in zip(a.iterate_state(), b.iterate_state()):
        assert np.array_equal(va, vb), name
    (xa, ya, ia), (xb, yb, ib) = a.solution(), b.solution()
    assert np.array_equal(xa, xb) and np.array_equal(ya, yb)
    assert [bytes(i) for i in ia] == [bytes(i) for i in ib], name


@pytest.mark.parametrize('name', NAMES)
def test_rollout_est_is_the_sequence_of_one_step_loops(name):
    import torch
    dev = torch.device('cuda:0')
    K = rc.CASES[name]['K']
    for own_plant, noisy in ((False, False), (True, True)):
        f = _forward(name, own_plant, noisy)
        tr = f['tr']
        assert np.all(tr['status'] == SOLVED)
        _same_forward(name, tr, f['seq'], f['Ka'], f['Kb'], f['esta'], f['estb'].x_true)
        assert np.array_equal(f['Kb'].x0_rh, f['Ka'].x0_rh) and np.array_equal(f['Kb'].uminus1_rh, f['Ka'].uminus1_rh) and np.array_equal(f['estb'].x, f['esta'].x)
        # the same with every buffer in device memory
        io = f['io']
        t = lambda a: None if a is None else torch.tensor(np.asarray(a, dtype=float), dtype=torch.float64, device=dev)
        Kd = _ctrl(name)
        B, nx, nu, ny = Kd.B, Kd.nx, Kd.nu, ec.ny_of(name)
        e64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
        out = [e64(K + 1, B, nx), e64(K, B, nu), i32(K, B), i32(K, B), e64(K + 1, B, nx), e64(K, B, ny)]
        xt = t(io['e']['x_true0'])
        Kd.prob.rollout_est(K, dict(C=t(io['e']['C']), L=t(io['e']['L']), x_true=xt, v=t(io['v'])), w=t(io['w']), Ap=t(io['Ap']), Bp=t(io['Bp']), out=out)
        Kd.prob.synchronize()
        for o, v in zip(out, ('x', 'u', 'status', 'iter', 'xhat', 'y')):
            assert np.array_equal(o.cpu().numpy(), tr[v]), (name, v)
        assert np.array_equal(xt.cpu().numpy(), f['estb'].x_true)
        for va, vb in zip(Kd.prob.iterate_state(), f['Kb'].prob.iterate_state()):
            assert np.array_equal(va, vb), name


def test_a_time_varying_reference_forward():
    name = 'first_tvref'
    seeds = rc.CASES[name]['seeds']
    K = rc.CASES[name]['K']
    io = _inputs(name, True, True, seeds)
    assert io['xref_traj'] is not None
    Ka, esta, seq, held = _twin(name, io, seeds)
    Kb = _ctrl(name, seeds)
    estb = _estimator(Kb, io['e'], v=io['v'])
    tr = Kb.rollout_est(K, estb, w=io['w'], Ap=io['Ap'], Bp=io['Bp'], xref_traj=io['xref_traj'])
    _same_forward(name, tr, seq, Ka, Kb, esta, estb.x_true)
    nx, nu = Kb.nx, Kb.nu
    for k in range(K):
        assert np.array_equal(Kb.prob.rollout_tape(k)['step'][:, nx + nu:], held[k]['xref']), k


# ---- 2. the tape --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_the_tape_is_what_the_twin_held_between_the_steps(name):
    for own_plant, noisy in ((False, False), (True, True)):
        f = _forward(name, own_plant, noisy)
        nx, nu = rc.CASES[name]['nx'], rc.CASES[name]['nu']
        for k, (e, h) in enumerate(zip(f['tape'], f['held'])):
            for v in ('x', 'z', 'y', 'status', 'x_plant', 'y_meas'):
                assert np.array_equal(e[v], h[v]), (name, k, v)
            assert np.array_equal(e['step'][:, :nx], h['x0']), (name, k)                # the estimate, not the plant state
            assert np.array_equal(e['step'][:, nx:nx + nu], h['um1']), (name, k)
            assert np.array_equal(e['step'][:, nx + nu:], h['xref']), (name, k)
            assert np.array_equal(e['x_plant'], f['tr']['x'][k]) and np.array_equal(e['y_meas'], f['tr']['y'][k])
    K = rc.CASES[name]['K']
    bp = f['Kb'].prob
    assert bp.rollout_tape_bytes(K, ny=ec.ny_of(name)) > bp.rollout_tape_bytes(K) > 0


# ---- 3. the reverse sweep against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ((False, False), (True, True)), ids=('model_quiet', 'plant_noisy'))
@pytest.mark.parametrize('name', NAMES)
def test_the_sweep_is_the_restatement(name, variant):
    f = _forward(name, *variant)
    Kb = f['Kb']
    for kind in ('xhuy', 'y'):
        g = _seeds(name, kind)
        got = _sweep(Kb, g, want=EVERY)
        assert np.all(got['status'] == 1) and np.all(got['n_weak'] == 0), (name, got['status'], got['n_weak'])
        errs = _compare(f, name, got, g, Kb)
        worst = max(errs.values())
        print('ROLLOUT_EST_ERR %s %s seeds %s: max %.3e  %s' % (name, variant, kind, worst, ' '.join('%s=%.1e' % kv for kv in errs.items())))
        assert worst <= TOL, (name, kind, errs)
        assert max(np.abs(got[k]).max() for k in ESTG) > 1e-3


# ---- 4. the factor reuse, and the same bits twice -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_reuse_changes_no_bit_and_saves_factorizations(name):
    f = _forward(name)
    Kb, K = f['Kb'], rc.CASES[name]['K']
    g = _seeds(name, 'xhuy')
    a = _sweep(Kb, g, want=EVERY)
    a2 = _sweep(Kb, g, want=EVERY)
    b = _sweep(Kb, g, want=EVERY, no_reuse=True)
    for k in EVERY + ('n_weak', 'status'):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], a2[k]), (name, k)
    assert np.array_equal(a['n_factor'], a2['n_factor']) and np.all(b['n_factor'] == K)
    print('ROLLOUT_EST_REUSE %s: n_factor %s of %d steps' % (name, a['n_factor'].tolist(), K))
    if name == ec.FIRST:
        n = a['n_factor'][ec.SEEDS[name].index(ec.REUSE_SEED)]
        assert 1 < n < K, a['n_factor']


# ---- 5. the older call on an estimator tape; one step written out ------------------------------------------------------------------------------
def test_rollout_adjoint_on_an_estimator_tape_is_the_call_without_estimator_io():
    from pympc_amd import _lib
    name = ec.FIRST
    f = _forward(name, True, True)
    Kb = f['Kb']
    bp = Kb.prob
    K, B, nx, nu = rc.CASES[name]['K'], Kb.B, Kb.nx, Kb.nu
    g = _seeds(name, 'xu')
    outs = []
    for est in (False, True):
        io = _lib.RolloutAdjointIO(); io.struct_size = C.sizeof(_lib.RolloutAdjointIO)
        io.G_x, io.G_u = g['x'].ctypes.data, g['u'].ctypes.data
        o = dict(lam=np.empty((K + 1, B, nx)), d_uminus1=np.empty((B, nu)), d_uref=np.empty((B, nu)), d_xref=np.empty((K, B, nx)), d_Ap=np.empty((B, nx, nx)), d_Bp=np.empty((B, nx, nu)))
        for k, a in o.items():
            setattr(io, k, a.ctypes.data)
        mo = _lib.AdjointModelIO(); mo.struct_size = C.sizeof(_lib.AdjointModelIO)
        o['d_Ad'] = np.empty((B, nx, nx)); mo.d_Ad = o['d_Ad'].ctypes.data
        rcode = bp._L.mpcqp_rollout_adjoint_est(bp._h, C.byref(io), None, C.byref(mo)) if est else bp._L.mpcqp_rollout_adjoint(bp._h, C.byref(io), C.byref(mo))
        assert rcode == 0
        outs.append(o)
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k
    via = _sweep(Kb, g, want=('lam', 'Ad'))
    assert np.array_equal(via['lam'], outs[0]['lam']) and np.array_equal(via['Ad'], outs[0]['d_Ad'])


@pytest.mark.parametrize('name', ('first', 'held', 'nb32_soft'))
def test_one_step_is_the_recursion_around_the_single_solve_adjoint(name):
    Kc = _ctrl(name)
    io = _inputs(name, True, True)
    e = io['e']
    Cm, L, Ad, Bd, Ap, Bp = e['C'], e['L'], Kc.Ad, Kc.Bd, io['Ap'], io['Bp']
    g = _seeds(name, 'xhuy')
    g = {k: v[:2] if k in ('x', 'xh') else v[:1] for k, v in g.items()}                  # K = 1
    T = lambda M: np.swapaxes(M, 1, 2)
    mv = lambda M, x: np.einsum('bij,bj->bi', M, x)
    lam1, eta1 = g['x'][1], g['xh'][1]
    gu0 = g['u'][0] + mv(T(Bp), lam1) + mv(T(Bd), eta1)
    one = Kc.adjoint(g_u0=gu0, want=('x0', 'uminus1', 'uref', 'xref') + MODEL)
    assert np.all(one['status'] == 1)
    u0 = Kc.prob.u0()
    est = _estimator(Kc, e, v=io['v'][:1])
    xh0, x0 = np.array(Kc.x0), np.array(e['x_true0'])
    tr = Kc.rollout_est(1, est, w=io['w'][:1], Ap=Ap, Bp=Bp)
    got = _sweep(Kc, g, want=EVERY)
    s = mv(T(Ad), eta1); t = mv(T(L), s); r = g['y'][0] + t
    inn = tr['y'][0] - mv(Cm, xh0)
    outer = lambda a, b: np.einsum('bi,bj->bij', a, b)
    want = dict(lam=np.stack([g['x'][0] + mv(T(Ap), lam1) + mv(T(Cm), r), lam1]), eta=np.stack([g['xh'][0] + s - mv(T(Cm), t) + one['x0'], eta1]),
                uminus1=one['uminus1'], uref=one['uref'], xref=one['xref'][None], Ap=outer(lam1, x0), Bp=outer(lam1, u0), C=outer(r, x0) - outer(t, xh0),
                L=outer(s, inn), v=r[None], Ae=outer(eta1, xh0 + mv(L, inn)), Be=outer(eta1, u0))
    want.update({k: one[k] for k in MODEL})
    for k in EVERY:
        assert _rel(got[k], want[k]) <= 1e-12, (name, k, _rel(got[k], want[k]))
    assert np.all(got['n_factor'] == 1)


# ---- 6. end to end: central differences of run(estimator=...) itself -----------------------------------------------------------------------
def test_the_sweep_against_central_differences_of_the_device_loop():
    """L = sum <Gx, x> + <Gxh, xhat> + <Gu, u> + <Gy, y> of run(K, estimator=...) on fresh controllers of 'first' / 0, in two entries each of
    L, C, xhat_0 and x_true0.  h = 1e-4 keeps the solver's 1e-9 below the bound; the loss is piecewise polynomial of low degree in these and
    the seed keeps every row 1e-3 away from a kink, so the truncation error is far below it too."""
    name, seeds = ec.FIRST, (0,)
    c = rc.CASES[name]
    K, nx, ny = c['K'], c['nx'], ec.ny_of(name)
    io = _inputs(name, False, True, seeds)
    g = _seeds(name, 'xhuy', B=1)
    Kb = _ctrl(name, seeds)
    Kb.rollout_est(K, _estimator(Kb, io['e'], v=io['v']), w=io['w'])
    got = _sweep(Kb, g, want=('lam', 'eta', 'C', 'L'))
    assert np.all(got['status'] == 1) and np.all(got['n_weak'] == 0)
    base = dict(L=io['e']['L'], C=io['e']['C'], xh0=rc.batch_kwargs(name, seeds)['x0'], x0=io['e']['x_true0'])

    def loss(p):
        Kc = _ctrl(name, seeds, over=dict(x0=p['xh0']))
        tr = Kc.run(K, estimator=_estimator(Kc, dict(C=p['C'], L=p['L'], x_true0=p['x0']), v=io['v']), w=io['w'])
        return float((g['x'] * tr['x']).sum() + (g['xh'] * tr['xhat']).sum() + (g['u'] * tr['u']).sum() + (g['y'] * tr['y']).sum())

    h = 1e-4
    entries = [('L', (0, 0, 0), got['L']), ('L', (0, nx - 1, ny - 1), got['L']), ('C', (0, 0, 1), got['C']), ('C', (0, ny - 1, nx - 1), got['C']),
               ('xh0', (0, 0), got['eta'][0]), ('xh0', (0, nx - 1), got['eta'][0]), ('x0', (0, 1), got['lam'][0]), ('x0', (0, 2), got['lam'][0])]
    fds = []
    for field, idx, grad in entries:
        vals = []
        for sgn in (1.0, -1.0):
            p = {k: np.array(v, dtype=float) for k, v in base.items()}
            p[field][idx] += sgn * h
            vals.append(loss(p))
        fd = (vals[0] - vals[1]) / (2 * h)
        fds.append(fd)
        print('ROLLOUT_EST_FD d/d%s%s: grad %+.6e fd %+.6e' % (field, list(idx[1:]), grad[idx], fd))
        assert abs(grad[idx] - fd) <= FD_TOL * max(1.0, abs(fd)), (field, idx, grad[idx], fd)
    assert max(abs(v) for v in fds) > 1e-2


# ---- 7. a failed step ----------------------------------------------------------------------------------------------------------------------
def test_a_failed_step_takes_the_not_solved_branch():
    name, seeds = ec.FIRST, (0, 3)
    K = rc.CASES[name]['K']
    Kc = _ctrl(name, seeds, max_iter=25)
    io = _inputs(name, False, True, seeds)
    tr = Kc.rollout_est(K, _estimator(Kc, io['e'], v=io['v']), w=io['w'])
    assert np.all(tr['status'][0] != SOLVED) and np.array_equal(tr['u'][0], Kc.uref)       # u_failure at step 0
    g = _seeds(name, 'xhuy', B=2)
    got = _sweep(Kc, g, want=EVERY)
    assert np.all(got['status'][0] == 0)
    f = dict(tape=[Kc.prob.rollout_tape(k) for k in range(K)], io=io, scaling=Kc.prob.scaling()[:3], refs={}, seeds=seeds)
    errs = _compare(f, name, got, g, Kc)
    assert max(errs.values()) <= TOL, errs
    if np.all(got['status'] == 0):                                                      # every step failed: nothing reaches u_{-1}, xref or the model
        for k in MODEL + ('uminus1', 'xref'):
            assert np.all(got[k] == 0.0), k


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from pympc_amd import _lib
    name, seeds = ec.FIRST, (0, 3)
    K = rc.CASES[name]['K']
    Kt = _ctrl(name, seeds)
    bp = Kt.prob
    L, h = bp._L, bp._h
    io = _inputs(name, False, True, seeds)
    e = io['e']
    g = _seeds(name, 'xhuy', B=2)
    state = lambda: [v.copy() for v in bp.iterate_state()] + [bp.solution()[0]]
    xt = e['x_true0'].copy()

    def loop(ny=2, Cm=e['C'], Lg=e['L'], x_true=xt):
        lo = _lib.Loop(); lo.ny = ny
        lo.C, lo.Lgain, lo.x_true = (None if a is None else a.ctypes.data for a in (Cm, Lg, x_true))
        return lo
    s0 = state()
    assert L.mpcqp_rollout_est(h, K, C.byref(loop(ny=0))) == -1                       # no estimator: that is mpcqp_rollout
    for miss in ('Cm', 'Lg', 'x_true'):
        assert L.mpcqp_rollout_est(h, K, C.byref(loop(**{miss: None}))) == -1, miss
    assert L.mpcqp_rollout(h, K, C.byref(loop())) == -4                               # the state-feedback rollout keeps refusing output feedback
    bp.update_settings(polish=True)
    assert L.mpcqp_rollout_est(h, K, C.byref(loop())) == -4                           # polishing on
    bp.update_settings(polish=False)
    Kt.update(Kt.x0, solve=False)
    assert L.mpcqp_rollout_est(h, K, C.byref(loop())) == -5                           # no solve behind the step data
    for a, b in zip(s0, state()):
        assert np.array_equal(a, b)
    assert np.array_equal(xt, e['x_true0'])
    sio = _lib.RolloutAdjointIO(); sio.struct_size = C.sizeof(_lib.RolloutAdjointIO); sio.G_u = g['u'].ctypes.data
    assert L.mpcqp_rollout_adjoint_est(h, C.byref(sio), None, None) == -5              # no tape yet
    assert L.mpcqp_rollout_get_tape_est(h, 0, None, None) == -5
    Kt.solve()
    # a state-feedback tape: the estimator's call, seeds and gradients are refused
    Kt.rollout(K)
    assert L.mpcqp_rollout_adjoint_est(h, C.byref(sio), None, None) == -5
    assert L.mpcqp_rollout_get_tape_est(h, 0, None, None) == -5
    with pytest.raises(RuntimeError, match='rollout_est'):
        Kt.rollout_adjoint(g_u=g['u'], g_y=g['y'])
    with pytest.raises(RuntimeError, match='rollout_est'):
        Kt.rollout_adjoint(g_u=g['u'], want=('lam', 'L'))
    assert 'x_plant' not in bp.rollout_tape(0)
    # an estimator tape
    Kt.update(rc.batch_kwargs(name, seeds)['x0'], rc.batch_kwargs(name, seeds)['uminus1'])
    Kt.rollout_est(K, _estimator(Kt, e, v=io['v']), w=io['w'])
    ref = _sweep(Kt, g, want=EVERY)
    s2 = state()
    eo = _lib.RolloutEstIO(); eo.struct_size = C.sizeof(_lib.RolloutEstIO); eo.G_y = g['y'].ctypes.data
    bad = _lib.RolloutEstIO(); bad.struct_size = C.sizeof(_lib.RolloutEstIO) - 8; bad.G_y = g['y'].ctypes.data
    none = _lib.RolloutAdjointIO(); none.struct_size = C.sizeof(_lib.RolloutAdjointIO)
    short = _lib.RolloutAdjointIO(); short.struct_size = C.sizeof(_lib.RolloutAdjointIO) - 8; short.G_u = g['u'].ctypes.data
    assert L.mpcqp_rollout_adjoint_est(h, C.byref(none), C.byref(bad), None) == -1    # wrong struct_size
    assert L.mpcqp_rollout_adjoint_est(h, C.byref(short), C.byref(eo), None) == -1
    assert L.mpcqp_rollout_adjoint_est(h, C.byref(none), None, None) == -1            # no seed
    empty = _lib.RolloutEstIO(); empty.struct_size = C.sizeof(_lib.RolloutEstIO)
    assert L.mpcqp_rollout_adjoint_est(h, C.byref(none), C.byref(empty), None) == -1
    assert L.mpcqp_rollout_adjoint_est(h, C.byref(none), C.byref(eo), None) == 0      # G_y alone is a seed
    with pytest.raises(ValueError):
        Kt.rollout_adjoint()
    with pytest.raises(RuntimeError, match=r'\(-1\)'):
        bp.rollout_tape(K)
    for a, b in zip(s2, state()):
        assert np.array_equal(a, b)
    again = _sweep(Kt, g, want=EVERY)
    for k in EVERY + ('n_factor',):
        assert np.array_equal(again[k], ref[k]), k
    bp.rollout_release()
    assert L.mpcqp_rollout_adjoint_est(h, C.byref(none), C.byref(eo), None) == -5     # released: no tape
    with pytest.raises(RuntimeError, match='no rollout'):
        Kt.rollout_adjoint(g_y=g['y'])
    with pytest.raises(TypeError):
        Kt.rollout(K, estimator=None)
    for a, b in zip(s2, state()):
        assert np.array_equal(a, b)


# ---- 9. state-feedback results do not move -------------------------------------------------------------------------------------------------
def test_the_state_feedback_sweep_is_the_same_before_and_after_an_estimator_rollout():
    name, seeds = ec.FIRST, (0, 3)
    K = rc.CASES[name]['K']
    a = rc.batch_kwargs(name, seeds)
    Kc = _ctrl(name, seeds)
    io = _inputs(name, False, True, seeds)
    g = _seeds(name, 'xu', B=2)
    bytes0 = Kc.prob.rollout_tape_bytes(K)
    res = []
    for rnd in range(2):
        tr = Kc.rollout(K, w=io['w'])
        sw = Kc.rollout_adjoint(g_x=g['x'], g_u=g['u'], want=CHAIN + MODEL)
        res.append((tr, sw))
        if rnd == 0:
            Kc.update(a['x0'], a['uminus1'])
            Kc.rollout_est(K, _estimator(Kc, io['e'], v=io['v']), w=io['w'])
            _sweep(Kc, _seeds(name, 'xhuy', B=2), want=EVERY)
            # the same problem set up again on the same handle: a cold start, so the loop below starts where the first one did
            Kc.prob.setup(a['Ad'], a['Bd'], a['Qx'], a['QxN'], a['Qu'], a['QDu'], a['xmin'], a['xmax'], a['umin'], a['umax'], a['Dumin'], a['Dumax'], a['uref'],
                          Kc.eps_feas, a['x0'], a['uminus1'], a['xref'])
            Kc.solve()
    for k in ('x', 'u', 'status', 'iter'):
        assert np.array_equal(res[0][0][k], res[1][0][k]), k
    for k in CHAIN + MODEL + ('n_factor', 'status'):
        assert np.array_equal(res[0][1][k], res[1][1][k]), k
    assert Kc.prob.rollout_tape_bytes(K) == bytes0


def test_the_state_feedback_sweep_on_what_an_estimator_rollout_left_on_the_handle():
    """Two controllers run the same output-feedback loop, one by rollout_est with its sweep (an estimator tape and the estimator kernel on
    its handle), one by K untaped run(1, estimator=...) calls -- the same bits, the iterate included (test 1).  Both are then updated to the
    same state and rolled out by state feedback: the trajectories and every output of rollout_adjoint are the same bits."""
    name, seeds = ec.FIRST, (0, 3)
    K = rc.CASES[name]['K']
    a = rc.batch_kwargs(name, seeds)
    io = _inputs(name, False, True, seeds)
    g = _seeds(name, 'xu', B=2)
    Ka, esta, _, _ = _twin(name, io, seeds)                # never held a tape
    Kb = _ctrl(name, seeds)
    Kb.rollout_est(K, _estimator(Kb, io['e'], v=io['v']), w=io['w'])
    _sweep(Kb, _seeds(name, 'xhuy', B=2), want=EVERY)
    res = []
    for Kc in (Ka, Kb):
        Kc.update(a['x0'], a['uminus1'])
        tr = Kc.rollout(K, w=io['w'])
        res.append((tr, Kc.rollout_adjoint(g_x=g['x'], g_u=g['u'], want=CHAIN + MODEL)))
    for k in ('x', 'u', 'status', 'iter'):
        assert np.array_equal(res[0][0][k], res[1][0][k]), k
    for k in CHAIN + MODEL + ('n_factor', 'status', 'n_weak'):
        assert np.array_equal(res[0][1][k], res[1][1][k]), k
    assert np.all(res[1][1]['status'] == 1)
    with pytest.raises(RuntimeError, match='rollout_est'):
        Kb.rollout_adjoint(g_u=g['u'], want=('eta',))      # (the tape is a state-feedback one again)


# ---- 10. torch -----------------------------------------------------------------------------------------------------------------------------
def test_mpc_rollout_est_is_one_sweep_with_the_matching_seeds():
    import torch
    from pympc_amd.torch_layer import mpc_rollout_est
    name = ec.FIRST
    c = rc.CASES[name]
    K, nx, nu, ny = c['K'], c['nx'], c['nu'], ec.ny_of(name)
    io = _inputs(name, True, True)
    e = io['e']
    dev = torch.device('cuda:0')
    t = lambda a, gr=True: torch.tensor(np.asarray(a, dtype=float), dtype=torch.float64, device=dev, requires_grad=gr)
    C1 = _ctrl(name)
    B = C1.B
    ins = dict(x0=t(e['x_true0']), xh0=t(C1.x0), C=t(e['C']), L=t(e['L']), v=t(io['v']), um1=t(C1.uminus1), xref=t(C1.xref), w=t(io['w']), Ap=t(io['Ap']), Bp=t(io['Bp']))
    params = dict(Ad=t(C1.Ad), Qx=t(C1.Qx[0]))
    X, XH, Y, U = mpc_rollout_est(C1, ins['x0'], ins['xh0'], K, ins['C'], ins['L'], v=ins['v'], u_prev=ins['um1'], xref=ins['xref'], w=ins['w'],
                                  Ap=ins['Ap'], Bp=ins['Bp'], params=params)
    assert X.shape == (K + 1, B, nx) and XH.shape == (K + 1, B, nx) and Y.shape == (K, B, ny) and U.shape == (K, B, nu) and Y.is_cuda
    g = _seeds(name, 'xhuy')
    wt = {k: torch.tensor(v, device=dev) for k, v in g.items()}
    loss = 0.5 * ((wt['x'] * X * X).sum() + (wt['xh'] * XH * XH).sum() + (wt['y'] * Y * Y).sum() + (wt['u'] * U * U).sum())
    grads = torch.autograd.grad(loss, list(ins.values()) + [params['Ad'], params['Qx']])
    C2 = _ctrl(name)
    C2.update_model(Ad=C1.Ad, Qx=np.broadcast_to(C1.Qx[0], C1.Qx.shape), solve=False)
    C2.update(C1.x0, C1.uminus1, C1.xref)
    tr = C2.rollout_est(K, _estimator(C2, e, v=io['v']), w=io['w'], Ap=io['Ap'], Bp=io['Bp'])
    for a, k in ((X, 'x'), (XH, 'xhat'), (Y, 'y'), (U, 'u')):
        assert np.array_equal(a.detach().cpu().numpy(), tr[k]), k
    ref = C2.rollout_adjoint(g_x=g['x'] * tr['x'], g_u=g['u'] * tr['u'], g_xhat=g['xh'] * tr['xhat'], g_y=g['y'] * tr['y'], want=EVERY)
    want = [ref['lam'][0], ref['eta'][0], ref['C'], ref['L'], ref['v'], ref['uminus1'], ref['xref'].sum(axis=0), ref['lam'][1:], ref['Ap'], ref['Bp'],
            ref['Ad'] + ref['Ae'], ref['Qx'].sum(axis=0)]
    for gr, w_, n in zip(grads, want, list(ins) + ['Ad', 'Qx']):
        assert tuple(gr.shape) == tuple(np.shape(w_)) and gr.is_cuda, n
        assert _rel(gr.cpu().numpy(), w_) <= 1e-13, (n, _rel(gr.cpu().numpy(), w_))
    # the plant is the model, L and C shared by the batch: Ad takes all three paths, shared tensors the batch sum
    C3 = _ctrl(name)
    pA, pB = t(C3.Ad[0]), t(C3.Bd[0])
    C3.update_model(Ad=np.broadcast_to(C3.Ad[0], C3.Ad.shape), Bd=np.broadcast_to(C3.Bd[0], C3.Bd.shape))
    tL, tC = t(e['L'][0]), t(e['C'][0])
    X, XH, Y, U = mpc_rollout_est(C3, t(e['x_true0'], False), t(C1.x0, False), K, tC, tL, params=dict(Ad=pA, Bd=pB))
    lossf = lambda X, XH, Y, U: 0.5 * ((wt['x'] * X * X).sum() + (wt['xh'] * XH * XH).sum() + (wt['y'] * Y * Y).sum() + (wt['u'] * U * U).sum())
    gA, gB, gL, gC = torch.autograd.grad(lossf(X, XH, Y, U), [pA, pB, tL, tC])
    sd = dict(g_x=(wt['x'] * X).detach(), g_u=(wt['u'] * U).detach(), g_xhat=(wt['xh'] * XH).detach(), g_y=(wt['y'] * Y).detach())
    per = C3.prob.rollout_adjoint(want=('Ad', 'Bd', 'Ap', 'Bp', 'Ae', 'Be', 'L', 'C'), **sd)
    assert per['L'].is_cuda
    for got_, parts in ((gA, ('Ad', 'Ap', 'Ae')), (gB, ('Bd', 'Bp', 'Be')), (gL, ('L',)), (gC, ('C',))):
        w_ = sum(per[p].sum(dim=0) for p in parts).cpu().numpy()
        assert _rel(got_.cpu().numpy(), w_) <= 1e-13, parts
    assert float(per['Ae'].abs().max()) > 1e-3
    # a second rollout between forward and backward is refused
    X, XH, Y, U = mpc_rollout_est(C3, t(e['x_true0']), t(C1.x0), K, tC, tL)
    C3.rollout(2)
    with pytest.raises(RuntimeError, match='rolled out again'):
        X.sum().backward()


def test_mpc_rollout_est_directional_derivative_in_L():
    """The gradcheck of L at 'first' / 0: central differences of the torch function along two random directions of L."""
    import torch
    from pympc_amd.torch_layer import mpc_rollout_est
    name, seeds = ec.FIRST, (0,)
    K = rc.CASES[name]['K']
    io = _inputs(name, False, True, seeds)
    e = io['e']
    dev = torch.device('cuda:0')
    t = lambda a, gr=False: torch.tensor(np.asarray(a, dtype=float), dtype=torch.float64, device=dev, requires_grad=gr)
    g = {k: t(v) for k, v in _seeds(name, 'xhuy', B=1).items()}
    Kc = _ctrl(name, seeds)
    xh0, um1 = np.array(Kc.x0), np.array(Kc.uminus1)

    def f(Lt):
        X, XH, Y, U = mpc_rollout_est(Kc, t(e['x_true0']), t(xh0), K, t(e['C']), Lt, v=t(io['v']), u_prev=t(um1), w=t(io['w']))
        return (g['x'] * X).sum() + (g['xh'] * XH).sum() + (g['y'] * Y).sum() + (g['u'] * U).sum()

    Lt = t(e['L'], True)
    grad, = torch.autograd.grad(f(Lt), Lt)
    rng = np.random.default_rng(31)
    h = 1e-4
    for _ in range(2):
        d = rng.standard_normal(e['L'].shape); d /= np.linalg.norm(d)
        fd = (f(t(e['L'] + h * d)).item() - f(t(e['L'] - h * d)).item()) / (2 * h)
        an = float((grad.cpu().numpy() * d).sum())
        print('ROLLOUT_EST_TORCH_FD: grad.d %+.6e fd %+.6e' % (an, fd))
        assert abs(an - fd) <= FD_TOL * max(1.0, abs(fd)), (an, fd)


# ---- 11. the example -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_differentiable_observer_example_lowers_the_cost():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'differentiable_observer.py'), '--batch', '32', '--steps', '12', '--iters', '20'],
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout)
    m = re.search(r'^OBSERVER_OK cost0 ([0-9.e+-]+) cost1 ([0-9.e+-]+)', r.stdout, flags=re.M)
    assert m, r.stdout
    assert float(m.group(2)) < float(m.group(1))
