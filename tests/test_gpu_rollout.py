"""The taped rollout and its reverse sweep on the device (include/mpcqp_rollout.h, pympc_amd/csrc/mpcqp_rollout.h) on the closed loops of
tests/rollout_cases.py: the trajectories and the handle against K one-step device loops, bit for bit; the tape against what those loops
held between the steps; the sweep against the numpy restatement tests/rollout_ref.py evaluated on the device's own tape and scaling;
K = 1 against mpcqp_adjoint_model; the factor reuse; central differences of run() itself; failed steps; state and errors; torch; the example.

Everything is solved at the project's parity setting eps_abs = eps_rel = 1e-9.  TOL and the central-difference bound are those of
tests/test_gpu_adjoint.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import rollout_cases as rc
import rollout_ref as rr
from rollout_dev import TOL, FD_TOL, SOLVED, CHAIN, ctrl as _ctrl, inputs as _inputs, forward as _forward, ref_tape as _ref_tape
from util import rel1_any as _rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODEL = rr.MODEL_NAMES
NAMES = sorted(rc.CASES)


def _reference(f, name, b, gx, gu):
    """The restatement's sweep of instance b on the device's tape (the Jacobians of the host builder and the QP of every entry made once)."""
    kw, attrs = rc.draw(name, rc.CASES[name]['seeds'][b])
    st = f['refs'].setdefault(b, {})
    tape = _ref_tape(f, name, b)
    if 'maps' not in st:
        st['maps'], st['cache'] = rr.adjoint_ref.parameter_maps(rr.entry_kwargs(kw, tape[0]), attrs), {}
    D, E, cs = f['scaling']
    io = f['io']
    return rr.sweep(kw, attrs, tape, D[b], E[b], cs[b], None if gx is None else gx[:, b], None if gu is None else gu[:, b],
                    Ap=None if io['Ap'] is None else io['Ap'][b], Bp=None if io['Bp'] is None else io['Bp'][b], maps=st['maps'], cache=st['cache'])


def _seeds(name, kind, B=None):
    c = rc.CASES[name]
    B = len(c['seeds']) if B is None else B
    rng = np.random.default_rng(23)
    gx, gu = rng.standard_normal((c['K'] + 1, B, c['nx'])), rng.standard_normal((c['K'], B, c['nu']))
    return (gx if 'x' in kind else None), (gu if 'u' in kind else None)


# ---- 1. trajectories and the handle afterwards --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_rollout_is_the_sequence_of_one_step_loops(name):
    for own_plant, with_w in ((False, False), (True, True)):
        f = _forward(name, own_plant, with_w)
        K, tr = rc.CASES[name]['K'], f['tr']
        for k in range(K):
            s = f['seq'][k]
            assert np.array_equal(tr['x'][k], s['x'][0]) and np.array_equal(tr['x'][k + 1], s['x'][1]), (name, k)
            assert np.array_equal(tr['u'][k], s['u'][0]) and np.array_equal(tr['status'][k], s['status'][0]) and np.array_equal(tr['iter'][k], s['iter'][0]), (name, k)
        assert np.all(tr['status'] == SOLVED)
        a, b = f['Ka'].prob, f['Kb'].prob
        for va, vb in zip(a.iterate_state(), b.iterate_state()):
            assert np.array_equal(va, vb), name
        (xa, ya, ia), (xb, yb, ib) = a.solution(), b.solution()
        assert np.array_equal(xa, xb) and np.array_equal(ya, yb)
        assert [bytes(i) for i in ia] == [bytes(i) for i in ib], name
        assert np.array_equal(f['Ka'].uminus1_rh, f['Kb'].uminus1_rh) and np.array_equal(f['Ka'].x0_rh, f['Kb'].x0_rh)


@pytest.mark.parametrize('name', NAMES)
def test_rollout_against_one_launch_of_all_steps(name):
    """run(K) in one launch against the taped rollout.  The sequence of one-step loops is what the rollout is by construction; whether ONE
    launch of K steps gives the same bits as K launches of one is a property of the device loop itself, compared here as it stands."""
    f = _forward(name, True, True)
    Kc = _ctrl(name)
    one = Kc.run(rc.CASES[name]['K'], **f['io'])
    for k in ('x', 'u', 'status', 'iter'):
        assert np.array_equal(one[k], f['tr'][k]), (name, k, np.abs(np.asarray(one[k], dtype=float) - f['tr'][k]).max())


# ---- 2. the tape --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_the_tape_is_what_the_handle_held_between_the_steps(name):
    for own_plant, with_w in ((False, False), (True, True)):
        f = _forward(name, own_plant, with_w)
        nx, nu = rc.CASES[name]['nx'], rc.CASES[name]['nu']
        for k, (e, h) in enumerate(zip(f['tape'], f['held'])):
            for v in ('x', 'z', 'y', 'status'):
                assert np.array_equal(e[v], h[v]), (name, k, v)
            assert np.array_equal(e['step'][:, :nx], h['x0']), (name, k)
            assert np.array_equal(e['step'][:, nx:nx + nu], h['um1']), (name, k)      # the u_{-1} the solve was made with
            assert np.array_equal(e['step'][:, nx + nu:], h['xref']), (name, k)
    assert f['Kb'].prob.rollout_tape_bytes(rc.CASES[name]['K']) > 0
    with pytest.raises(RuntimeError, match=r'\(-1\)'):
        f['Kb'].prob.rollout_tape(rc.CASES[name]['K'])


# ---- 3. the reverse sweep against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_w', (False, True), ids=('no_w', 'w'))
@pytest.mark.parametrize('own_plant', (False, True), ids=('plant_is_model', 'plant_given'))
@pytest.mark.parametrize('name', NAMES)
def test_the_sweep_is_the_restatement(name, own_plant, with_w):
    f = _forward(name, own_plant, with_w)
    Kb = f['Kb']
    K = rc.CASES[name]['K']
    for kind in ('x', 'u', 'xu'):
        gx, gu = _seeds(name, kind)
        got = Kb.rollout_adjoint(g_x=gx, g_u=gu, want=CHAIN + MODEL)
        nact, nweak, status, nfac = Kb.prob.rollout_info()
        assert np.all(status == 1) and np.all(nweak == 0), (name, status, nweak)
        errs = {}
        for b in range(Kb.B):
            ref = _reference(f, name, b, gx, gu)
            assert np.array_equal(nact[:, b], ref['n_active']) and np.array_equal(nweak[:, b], ref['n_weak']), (name, b, nact[:, b], ref['n_active'])
            assert nfac[b] == ref['n_factor'], (name, b, nfac[b], ref['n_factor'])
            for k in CHAIN + MODEL:
                v = got[k][:, b] if k in ('lam', 'xref') else got[k][b]
                errs[k] = max(errs.get(k, 0.0), _rel(v, ref[k]))
        worst = max(errs.values())
        print('ROLLOUT_ERR %s plant %s w %s seeds %s: max %.3e  %s' % (name, 'given' if own_plant else 'model', with_w, kind, worst,
                                                                      ' '.join('%s=%.1e' % kv for kv in errs.items())))
        assert worst <= TOL, (name, kind, errs)
    assert got['n_factor'].shape == (Kb.B,) and got['status'].shape == (K, Kb.B)


# ---- 4. one step is mpcqp_adjoint_model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ('first', 'held', 'nb32_soft'))
def test_one_step_with_no_state_seed_is_the_single_solve_adjoint(name):
    K = _ctrl(name)
    g = np.random.default_rng(3).standard_normal((K.B, K.nu))
    one = K.adjoint(g_u0=g, want=('x0', 'uminus1', 'uref', 'xref') + MODEL)
    assert np.all(one['status'] == 1)
    K.rollout(1)
    got = K.rollout_adjoint(g_u=g[None], want=CHAIN + MODEL)
    pairs = [('lam', got['lam'][0], one['x0']), ('uminus1', got['uminus1'], one['uminus1']), ('uref', got['uref'], one['uref']), ('xref', got['xref'][0], one['xref'])]
    pairs += [(k, got[k], one[k]) for k in MODEL]
    for k, a, b in pairs:
        assert _rel(a, b) <= 1e-12, (name, k, _rel(a, b))
    assert np.all(got['lam'][1] == 0.0) and np.all(got['n_factor'] == 1)


# ---- 5. the factor reuse ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_reuse_changes_no_bit_and_saves_factorizations(name):
    f = _forward(name)
    Kb, K = f['Kb'], rc.CASES[name]['K']
    gx, gu = _seeds(name, 'xu')
    a = Kb.rollout_adjoint(g_x=gx, g_u=gu, want=CHAIN + MODEL)
    b = Kb.rollout_adjoint(g_x=gx, g_u=gu, want=CHAIN + MODEL, no_reuse=True)
    for k in CHAIN + MODEL + ('n_weak', 'status'):
        assert np.array_equal(a[k], b[k]), (name, k)
    counts = [_reference(f, name, i, gx, gu) for i in range(Kb.B)]
    assert np.array_equal(a['n_factor'], [r['n_factor'] for r in counts]), (name, a['n_factor'])
    assert np.array_equal(b['n_factor'], [r['n_solved'] for r in counts]) and np.all(b['n_factor'] == K)
    print('ROLLOUT_REUSE %s: n_factor %s of %d steps' % (name, a['n_factor'].tolist(), K))
    if name == rc.FIRST:
        assert np.any((a['n_factor'] > 1) & (a['n_factor'] < K)), a['n_factor']


# ---- 6. end to end: central differences of run() itself ------------------------------------------------------------------------------------
def test_the_sweep_against_central_differences_of_the_device_loop():
    """L = sum <Gx[k], x_k> + sum <Gu[k], u_k> of run(K) on fresh controllers, in two directions of x0 and two of Ad (plant = model: the
    direction moves the plant too, d_Ad + d_Ap).  The control law is piecewise affine and the listed seeds keep every row 1e-3 away from a
    kink, so the step h = 1e-4 makes no truncation error and keeps the solver's 1e-9 below the bound."""
    name = rc.FIRST
    c = rc.CASES[name]
    K, B = c['K'], len(c['seeds'])
    gx, gu = _seeds(name, 'xu')
    f = _forward(name)
    got = f['Kb'].rollout_adjoint(g_x=gx, g_u=gu, want=('lam', 'Ap', 'Ad'))
    assert np.all(got['status'] == 1) and np.all(got['n_weak'] == 0)
    base = rc.batch_kwargs(name)
    rng = np.random.default_rng(29)
    h = 1e-4

    def loss(over):
        tr = _ctrl(name, over=over).run(K)
        return (gx * tr['x']).sum(axis=(0, 2)) + (gu * tr['u']).sum(axis=(0, 2))      # per instance: they are independent

    for field, grad in (('x0', got['lam'][0]), ('Ad', got['Ad'] + got['Ap'])):
        for _ in range(2):
            d = rng.standard_normal(base[field].shape)
            d /= np.sqrt((d * d).reshape(B, -1).sum(axis=1)).reshape((B,) + (1,) * (d.ndim - 1))
            fd = (loss({field: base[field] + h * d}) - loss({field: base[field] - h * d})) / (2 * h)
            an = (grad * d).reshape(B, -1).sum(axis=1)
            err = np.abs(an - fd).max()
            print('ROLLOUT_FD d/d%s: |grad.d - FD|_inf = %.3e, |FD|_inf = %.3e' % (field, err, np.abs(fd).max()))
            assert err <= FD_TOL * max(1.0, np.abs(fd).max()), (field, err, an, fd)
            assert np.abs(fd).max() > 1e-2


# ---- 7. failed steps -----------------------------------------------------------------------------------------------------------------------
def _plant_alone(gx, gu, A, Bm):
    K = gu.shape[0]
    lam = np.zeros_like(gx); lam[K] = gx[K]
    dur = np.zeros_like(gu[0])
    for k in range(K - 1, -1, -1):
        dur += gu[k] + lam[k + 1] @ Bm
        lam[k] = gx[k] + lam[k + 1] @ A
    return lam, dur


def test_a_loop_whose_every_solve_fails_passes_through_the_plant_alone():
    name = rc.FIRST
    K = rc.CASES[name]['K']
    C = _ctrl(name, seeds=(0, 3), max_iter=25)
    tr = C.rollout(K)
    assert np.all(tr['status'] != SOLVED) and set(C.status()) == {'maximum iterations reached'}
    assert np.array_equal(tr['u'], np.broadcast_to(C.uref, tr['u'].shape))             # u_failure
    gx, gu = _seeds(name, 'xu', B=2)
    got = C.rollout_adjoint(g_x=gx, g_u=gu, want=CHAIN + MODEL)
    assert np.all(got['status'] == 0) and np.all(got['n_factor'] == 0)
    for b in range(2):
        lam, dur = _plant_alone(gx[:, b], gu[:, b], C.Ad[b], C.Bd[b])
        assert _rel(got['lam'][:, b], lam) <= 1e-13 and _rel(got['uref'][b], dur) <= 1e-13
    for k in MODEL + ('uminus1', 'xref'):
        assert np.all(got[k] == 0.0), k


def _held_to_the_restatement(C, name, io, gx, gu, got):
    """Every instance of a swept controller against the restatement on its own tape, failed entries included."""
    K = rc.CASES[name]['K']
    f = dict(tape=[C.prob.rollout_tape(k) for k in range(K)], io=io, scaling=C.prob.scaling()[:3], refs={})
    for b in range(C.B):
        ref = _reference(f, name, b, gx, gu)
        assert np.array_equal(got['status'][:, b], ref['status']) and got['n_factor'][b] == ref['n_factor'], (b, got['status'][:, b], got['n_factor'][b])
        for k in CHAIN + MODEL:
            v = got[k][:, b] if k in ('lam', 'xref') else got[k][b]
            assert _rel(v, ref[k]) <= TOL, (b, k, _rel(v, ref[k]))
    return np.array([e['status'] for e in f['tape']])


def test_a_failed_first_step_beside_solved_instances():
    """An instance whose u_{-1} lies so far outside the input box that the first Delta-u rows cannot be met: its solve for x_0 is primal
    infeasible, u_failure = uref is applied, and every later step solves.  Its tape mixes a failed entry with solved ones; all instances,
    this one included, are the restatement's."""
    name = rc.FIRST
    K = rc.CASES[name]['K']
    um1 = rc.batch_kwargs(name)['uminus1'].copy(); um1[1] = 5.0
    C = _ctrl(name, over=dict(uminus1=um1))
    tr = C.rollout(K)
    gx, gu = _seeds(name, 'xu')
    got = C.rollout_adjoint(g_x=gx, g_u=gu, want=CHAIN + MODEL)
    taped = _held_to_the_restatement(C, name, dict(Ap=None, Bp=None), gx, gu, got)
    assert taped[0, 1] != SOLVED and np.all(taped[1:, 1] == SOLVED) and np.all(np.delete(taped, 1, axis=1) == SOLVED), taped
    assert np.array_equal(tr['u'][0, 1], C.uref[1]) and np.all(got['uminus1'][1] == 0.0)      # u_failure; nothing reaches the u_{-1} behind a failed step
    assert np.all(got['n_weak'] == 0)


def test_a_failed_step_in_the_middle_of_a_tape():
    """The hard-box case with a disturbance that throws the first instance's state out of its box for one step: entry 1 of its tape is
    primal infeasible between solved entries, so the sweep carries lam through the plant alone there, restarts mu at zero, and goes on with
    the factor and the active set it had before.  Every instance against the restatement."""
    name = 'hard'
    c = rc.CASES[name]
    K = c['K']
    x1 = _ctrl(name).run(1)['x'][1]
    w = np.zeros((K, len(c['seeds']), c['nx'])); w[0, 0, 0] = 6.0 - x1[0, 0]      # x_1[0] = 6 against a box of 4
    C = _ctrl(name)
    C.rollout(K, w=w)
    gx, gu = _seeds(name, 'xu')
    got = C.rollout_adjoint(g_x=gx, g_u=gu, want=CHAIN + MODEL)
    taped = _held_to_the_restatement(C, name, dict(Ap=None, Bp=None), gx, gu, got)
    assert taped[:, 0].tolist() == [SOLVED, taped[1, 0], SOLVED, SOLVED] and taped[1, 0] != SOLVED, taped[:, 0]
    assert np.all(taped[:, 1:] == SOLVED) and np.all(got['n_weak'] == 0)


# ---- 8. state and errors -------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    import ctypes as C
    from pympc_amd import _lib
    name = rc.FIRST
    c = rc.CASES[name]
    K, nx, nu = c['K'], c['nx'], c['nu']
    Kt = _ctrl(name, seeds=(0, 3))
    bp = Kt.prob
    gx, gu = _seeds(name, 'xu', B=2)
    L, h = bp._L, bp._h
    io = _lib.RolloutAdjointIO(); io.struct_size = C.sizeof(_lib.RolloutAdjointIO)
    io.G_u = gu.ctypes.data
    assert L.mpcqp_rollout_adjoint(h, C.byref(io), None) == -5                      # before any rollout
    assert L.mpcqp_get_rollout_info(h, None, None, None, None) == -5
    assert L.mpcqp_rollout_get_tape(h, 0, None, None, None, None, None) == -5
    state = lambda: [v.copy() for v in bp.iterate_state()] + [bp.solution()[0]]
    s0 = state()
    lo = _lib.Loop(); lo.ny = 2
    assert L.mpcqp_rollout(h, K, C.byref(lo)) == -4                                 # output feedback
    bp.update_settings(polish=True)
    assert L.mpcqp_rollout(h, K, C.byref(_lib.Loop())) == -4                        # polishing on
    bp.update_settings(polish=False)
    for a, b in zip(s0, state()):
        assert np.array_equal(a, b)
    Kt.update(Kt.x0, solve=False)
    assert L.mpcqp_rollout(h, K, C.byref(_lib.Loop())) == -5                        # no solve behind the step data
    for a, b in zip(s0, state()):
        assert np.array_equal(a, b)
    assert L.mpcqp_rollout_adjoint(h, C.byref(io), None) == -5                      # (and still no tape)
    Kt.solve()
    s1 = state()
    with pytest.raises(NotImplementedError):                                          # a time-varying reference of another shape than the controller's
        Kt.rollout(K, xref_traj=np.zeros((K, 2, (c['Np'] + 1) * nx)))
    for a, b in zip(s1, state()):
        assert np.array_equal(a, b)
    assert L.mpcqp_rollout_adjoint(h, C.byref(io), None) == -5
    tr = Kt.rollout(K)
    ref = Kt.rollout_adjoint(g_x=gx, g_u=gu, want=CHAIN + MODEL)
    bad = _lib.RolloutAdjointIO(); bad.struct_size = C.sizeof(_lib.RolloutAdjointIO) - 8; bad.G_u = gu.ctypes.data
    assert L.mpcqp_rollout_adjoint(h, C.byref(bad), None) == -1                     # wrong struct_size
    none = _lib.RolloutAdjointIO(); none.struct_size = C.sizeof(_lib.RolloutAdjointIO)
    assert L.mpcqp_rollout_adjoint(h, C.byref(none), None) == -1                    # no seed
    mo = _lib.AdjointModelIO(); mo.struct_size = 4
    assert L.mpcqp_rollout_adjoint(h, C.byref(io), C.byref(mo)) == -1
    # q alone in raw-vector mode: the rollout refuses as the loop does and changes nothing; the tape, which reads no q, is still good
    _, q, _, l, u = bp.export_qp()
    bp.update_vectors(q)
    s2 = state()
    assert L.mpcqp_rollout(h, K, C.byref(_lib.Loop())) == -5
    for a, b in zip(s2, state()):
        assert np.array_equal(a, b)
    Kt.update(tr['x'][-1], tr['u'][-1])                                              # (back to the controller's own vectors, and a solve)
    # the tape is a copy: steps and solves in between change no bit of the sweep, and two sweeps of one tape are the same bits
    Kt.step(tr['x'][-1] * 0.9)
    Kt.solve()
    for again in (Kt.rollout_adjoint(g_x=gx, g_u=gu, want=CHAIN + MODEL), Kt.rollout_adjoint(g_x=gx, g_u=gu, want=CHAIN + MODEL)):
        for k in CHAIN + MODEL + ('n_factor',):
            assert np.array_equal(again[k], ref[k]), k
    s1 = Kt.rollout_adjoint(g_x=gx, g_u=gu, want=MODEL, batch_sum=True)
    s2 = Kt.rollout_adjoint(g_x=gx, g_u=gu, want=MODEL, batch_sum=True)
    for k in MODEL:
        assert s1[k].shape[0] == 1 and np.array_equal(s1[k], s2[k]), k
        assert _rel(s1[k][0], ref[k].sum(axis=0)) <= 1e-13, k
    # a solve after the sweep is the solve without it
    Ku, Kv = _ctrl(name, seeds=(0, 3)), _ctrl(name, seeds=(0, 3))
    for ctl in (Ku, Kv):
        ctl.rollout(K)
    Ku.rollout_adjoint(g_x=gx, g_u=gu, want=CHAIN + MODEL)
    for ctl in (Ku, Kv):
        ctl.update(tr['x'][2], tr['u'][1])
    for a, b in zip(Ku.prob.iterate_state(), Kv.prob.iterate_state()):
        assert np.array_equal(a, b)
    assert [bytes(i) for i in Ku.prob.infos()] == [bytes(i) for i in Kv.prob.infos()]
    # a new model under the handle: the tape was made under another one
    Ku.update_model(Ad=Ku.Ad * 0.99)
    with pytest.raises(RuntimeError, match=r'\(-5\)'):
        Ku.rollout_adjoint(g_x=gx, g_u=gu)
    Ku.rollout(K)
    assert np.all(Ku.rollout_adjoint(g_x=gx, g_u=gu)['status'] == 1)
    # new bounds through the raw-vector seam are decoded into the model blob the sweep reads: the tape is no longer good
    _, q, _, l, u = Ku.prob.export_qp()
    Ku.prob.update_vectors(None, np.clip(l, -1e30, 1e30), np.clip(u, -1e30, 1e30))
    with pytest.raises(RuntimeError, match=r'\(-5\)'):
        Ku.rollout_adjoint(g_x=gx, g_u=gu)
    Ku.update(tr['x'][0], tr['u'][0]); Ku.rollout(K)
    assert np.all(Ku.rollout_adjoint(g_x=gx, g_u=gu)['status'] == 1)
    Ku.prob.rollout_release()
    assert L.mpcqp_rollout_adjoint(Ku.prob._h, C.byref(io), None) == -5               # released: no tape
    with pytest.raises(RuntimeError, match='no rollout'):
        Ku.rollout_adjoint(g_x=gx, g_u=gu)
    with pytest.raises(TypeError):
        Kv.rollout(K, estimator=None)                                                # (no estimator, no model schedule: not in the signature)


def test_a_new_setup_invalidates_the_tape():
    """The sweep reads the model blob and the scaling from the handle, and every setup call rewrites them (launch_setup): setup again --
    through the controller data and through the raw-vector seam -- and the tape made before it is refused until the loop is rolled out again."""
    name = rc.FIRST
    K = rc.CASES[name]['K']
    C = _ctrl(name, seeds=(0, 3))
    gx, gu = _seeds(name, 'xu', B=2)
    C.rollout(K)
    ref = C.rollout_adjoint(g_x=gx, g_u=gu, want=CHAIN + MODEL)
    bp = C.prob
    a = rc.batch_kwargs(name, (0, 3))
    _, q, _, l, u = bp.export_qp()
    bp.setup(a['Ad'], a['Bd'], a['Qx'], a['QxN'], a['Qu'], a['QDu'], a['xmin'], a['xmax'], a['umin'], a['umax'], a['Dumin'], a['Dumax'], a['uref'],
             C.eps_feas, a['x0'], a['uminus1'], a['xref'])                    # mpcqp_setup on the handle that holds the tape
    with pytest.raises(RuntimeError, match=r'\(-5\)'):
        C.rollout_adjoint(g_x=gx, g_u=gu)
    assert bp.rollout_tape(0)['x'].shape == (2, bp.n)                                # (the entries can still be read; they are not differentiated)
    C.solve()
    C.rollout(K)
    again = C.rollout_adjoint(g_x=gx, g_u=gu, want=CHAIN + MODEL)
    for k in CHAIN + MODEL:                                                          # the same problem set up again: the same loop, the same sweep
        assert np.array_equal(again[k], ref[k]), k
    bp.setup_qp(a['Ad'], a['Bd'], a['Qx'], a['QxN'], a['Qu'], a['QDu'], C.eps_feas, q, np.clip(l, -1e30, 1e30), np.clip(u, -1e30, 1e30), uref=a['uref'])
    with pytest.raises(RuntimeError, match=r'\(-5\)'):                               # mpcqp_setup_qp
        C.rollout_adjoint(g_x=gx, g_u=gu)
    C.update(a['x0'], a['uminus1'], a['xref'])                                       # back to the controller's own vectors, and a solve
    C.rollout(K)
    assert np.all(C.rollout_adjoint(g_x=gx, g_u=gu)['status'] == 1)


# ---- 9. torch ------------------------------------------------------------------------------------------------------------------------------
def test_mpc_rollout_is_one_sweep_with_the_matching_seeds():
    import torch
    from pympc_amd.torch_layer import mpc_rollout
    name = rc.FIRST
    c = rc.CASES[name]
    K, nx, nu = c['K'], c['nx'], c['nu']
    io = _inputs(name, True, True)
    dev = torch.device('cuda:0')
    t = lambda a, g=True: torch.tensor(np.asarray(a, dtype=float), dtype=torch.float64, device=dev, requires_grad=g)
    C1 = _ctrl(name)
    B = C1.B
    tx, tu, tr, tw, tA, tB = t(C1.x0), t(C1.uminus1), t(C1.xref), t(io['w']), t(io['Ap']), t(io['Bp'])
    params = dict(Ad=t(C1.Ad), Qx=t(C1.Qx[0]))              # one per instance, one shared
    X, U = mpc_rollout(C1, tx, K, u_prev=tu, xref=tr, w=tw, Ap=tA, Bp=tB, params=params)
    assert X.shape == (K + 1, B, nx) and U.shape == (K, B, nu) and X.is_cuda
    wx, wu = torch.tensor(_seeds(name, 'xu')[0], device=dev), torch.tensor(_seeds(name, 'xu')[1], device=dev)
    loss = 0.5 * (wx * X * X).sum() + 0.5 * (wu * U * U).sum()
    ins = [tx, tu, tr, tw, tA, tB, params['Ad'], params['Qx']]
    grads = torch.autograd.grad(loss, ins)
    # the same forward without torch, and the sweep with the seeds the loss implies
    C2 = _ctrl(name)
    C2.update_model(Ad=C1.Ad, Qx=np.broadcast_to(C1.Qx[0], C1.Qx.shape), solve=False)
    C2.update(C1.x0, C1.uminus1, C1.xref)
    ref_tr = C2.rollout(K, w=io['w'], Ap=io['Ap'], Bp=io['Bp'])
    assert np.array_equal(X.detach().cpu().numpy(), ref_tr['x']) and np.array_equal(U.detach().cpu().numpy(), ref_tr['u'])
    gx, gu = wx.cpu().numpy() * ref_tr['x'], wu.cpu().numpy() * ref_tr['u']
    ref = C2.rollout_adjoint(g_x=gx, g_u=gu, want=CHAIN + ('Ad', 'Qx'))
    want = [ref['lam'][0], ref['uminus1'], ref['xref'].sum(axis=0), ref['lam'][1:], ref['Ap'], ref['Bp'], ref['Ad'], ref['Qx'].sum(axis=0)]
    for g, w_, n in zip(grads, want, ('x0', 'u_prev', 'xref', 'w', 'Ap', 'Bp', 'Ad', 'Qx')):
        assert tuple(g.shape) == tuple(np.shape(w_)) and g.is_cuda, n
        assert _rel(g.cpu().numpy(), w_) <= 1e-13, (n, _rel(g.cpu().numpy(), w_))
    # plant = the controller's own model: the Ad gradient carries the plant path; shared parameters take the device's batch sum
    C3 = _ctrl(name)
    pA, pB = t(C3.Ad[0]), t(C3.Bd[0])
    C3.update_model(Ad=np.broadcast_to(C3.Ad[0], C3.Ad.shape), Bd=np.broadcast_to(C3.Bd[0], C3.Bd.shape))
    X, U = mpc_rollout(C3, t(C1.x0, False), K, params=dict(Ad=pA, Bd=pB))
    gA, gB = torch.autograd.grad(0.5 * (wx * X * X).sum() + 0.5 * (wu * U * U).sum(), [pA, pB])
    gx, gu = (wx * X).detach(), (wu * U).detach()
    dev_res = C3.prob.rollout_adjoint(g_x=gx, g_u=gu, want=('Ad', 'Bd', 'Ap', 'Bp'), batch_sum=True)
    assert dev_res['Ad'].is_cuda and dev_res['Ad'].shape == (1, nx, nx)              # device in, device out
    assert torch.equal(gA, dev_res['Ad'][0] + dev_res['Ap'].sum(dim=0)) and torch.equal(gB, dev_res['Bd'][0] + dev_res['Bp'].sum(dim=0))
    per = C3.prob.rollout_adjoint(g_x=gx, g_u=gu, want=('Ad', 'Ap'))
    assert _rel(gA.cpu().numpy(), (per['Ad'] + per['Ap']).sum(dim=0).cpu().numpy()) <= 1e-13
    assert float(dev_res['Ap'].abs().max()) > 1e-3                                  # (a path that is there)
    # stepping in between is fine (the tape is a copy), a second rollout is not
    X, U = mpc_rollout(C3, t(C1.x0), K)
    C3.step(C1.x0)
    X.sum().backward()
    X, U = mpc_rollout(C3, t(C1.x0), K)
    C3.rollout(2)
    with pytest.raises(RuntimeError, match='rolled out again'):
        X.sum().backward()


def test_mpc_rollout_on_the_controllers_stream_makes_no_host_round_trip():
    """Every pointer of the two library calls is a device pointer: forward and backward are stream-ordered on torch's stream."""
    import torch
    from pympc_amd.torch_layer import mpc_rollout
    name = rc.FIRST
    K = rc.CASES[name]['K']
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        C1 = _ctrl(name, over=dict(stream=stream.cuda_stream))
        dev = torch.device('cuda:0')
        tx = torch.tensor(C1.x0, dtype=torch.float64, device=dev, requires_grad=True)
        seen = []
        orig = C1.prob.rollout_adjoint

        def spy(**kw):
            seen.append(all(v is None or (hasattr(v, 'is_cuda') and v.is_cuda) for v in (kw.get('g_x'), kw.get('g_u'))))
            res = orig(**kw)
            seen.append(all(v.is_cuda for v in res.values()))
            return res
        C1.prob.rollout_adjoint = spy
        X, U = mpc_rollout(C1, tx, K)
        (X[-1] ** 2).sum().backward()
        assert seen == [True, True] and tx.grad is not None and tx.grad.is_cuda
    stream.synchronize()
    C2 = _ctrl(name)
    C2.update(C1.x0)
    tr = C2.rollout(K)
    gx = np.zeros_like(tr['x']); gx[-1] = 2 * tr['x'][-1]
    assert _rel(tx.grad.cpu().numpy(), C2.rollout_adjoint(g_x=gx, want=('lam',))['lam'][0]) <= 1e-13


# ---- 10. the example -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_differentiable_rollout_example_descends():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'differentiable_rollout.py'), '--batch', '64', '--steps', '8', '--iters', '6'],
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout)
    loss = [float(v) for v in re.findall(r'^iteration +\d+: loss ([0-9.e+-]+)', r.stdout, flags=re.M)]
    assert len(loss) == 7, r.stdout
    assert all(b < a for a, b in zip(loss, loss[1:])), loss
    ratio = [float(v) for v in re.findall(r'decrease / predicted ([0-9.e+-]+)', r.stdout)]      # (the first line, before any step, prints nan)
    assert len(ratio) == 6 and all(0.25 <= v <= 1.25 for v in ratio), ratio      # it falls by what the gradient says (the example's Armijo rule)
    per_step = [float(v) for v in re.findall(r'factorizations per step ([0-9.]+)', r.stdout)]
    assert per_step and all(0.0 < v <= 1.0 for v in per_step), per_step
