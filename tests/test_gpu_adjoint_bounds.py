"""The bound gradients on the device (include/mpcqp_adjoint_bounds.h, pympc_amd/csrc/mpcqp_adjoint_bounds.h) on the table of
tests/bounds_cases.py: the single solve and the two sweeps against the numpy restatement tests/bounds_ref.py evaluated on the device's own
iterate / tape; K = 1 against the single solve; central differences of run() itself; bit-identity with the older calls, of repeated calls,
of the factor reuse and of a later solve; the batch sum; zeros and refusals; torch.autograd through mpc_step, mpc_rollout and
mpc_rollout_est with ``bounds=``; the example.

Everything is solved at the project's parity setting eps_abs = eps_rel = 1e-9.  TOL and the central-difference bounds are those of
tests/test_gpu_adjoint.py, tests/test_gpu_rollout.py and tests/test_gpu_rollout_est.py (they live in tests/adjoint_cases.py and
tests/rollout_dev.py)."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import adjoint_cases as ac
import adjoint_ref as ar
import adjoint_model_ref as am
import bounds_cases as bc
import bounds_ref as br
import rollout_cases as rc
import rollout_est_cases as ec
import rollout_dev as rd
import rollout_ref as rr
import util
from adjoint_cases import TOL, EPS, RAW, CHAINED
from rollout_dev import FD_TOL, SOLVED, CHAIN
from util import rel1_any as _rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = br.NAMES
MODEL = am.NAMES
SHAPES = ('nb16_nu7_hard', 'nb32_nu9_held', 'nb64_nu6', 'nb128_nu5', 'long100_nu2')      # every NB, a held input, no slack: the first seed of each
assert TOL == rd.TOL


# ---- 1. the single solve against the restatement ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _single(name):
    """One solve on the device and ONE call for l, u and the six bound gradients (made once, read-only afterwards)."""
    if name in ac.CASES:
        kw, attrs = ac.draw(name, ac.CASES[name]['seeds'][0])
        bp = ac.case_batch(name, ac.CASES[name]['seeds'][:1]).prob
    else:
        kw, attrs = bc.single(name)
        k2 = util.KW(kw); k2.attrs = attrs
        bp = ac.solved(k2).prob.batch_problem
    g = np.random.default_rng(7).standard_normal((bp.batch, bp.n))
    got = bp.adjoint(g_w=g, want=RAW + BOUNDS)
    return bp, g, got, bp.adjoint_info(), kw, attrs


@pytest.mark.parametrize('name', bc.SINGLE + SHAPES)
def test_the_single_solve_is_the_restatement_on_the_devices_iterate(name):
    bp, g, got, (nact, nweak, status), kw, attrs = _single(name)
    st = ac.device_state(bp)
    ref = ar.adjoint(*st, g[0])
    assert status[0] == 1 and nweak[0] == 0 and ref['n_weak'] == 0 and nact[0] == ref['n_active'], (name, status, nweak, nact, ref['n_active'])
    maps = br.bound_maps(kw, attrs)
    want, own = br.step(maps, ref), br.chain(maps, got['l'][0], got['u'][0])
    errs = {k: (_rel(got[k][0], want[k]), _rel(got[k][0], own[k])) for k in BOUNDS}
    print('BOUNDS_ERR %s: %s' % (name, '  '.join('%s %.1e/%.1e of %.1e' % (k, e[0], e[1], np.abs(want[k]).max()) for k, e in errs.items())))
    for k in BOUNDS:
        assert got[k].shape == (1, bp.nx if k in ('xmin', 'xmax') else bp.nu), k
        assert max(errs[k]) <= TOL, (name, k, errs[k])
    assert max(np.abs(want[k]).max() for k in BOUNDS) > 1e-6, name       # (something is active)
    if name == bc.HARD_STATE:
        assert np.abs(got['xmax'][0]).max() > 1e-6 and bp.n == (bp.Np + 1) * bp.nx + bp.Nc * bp.nu      # an active state row without slack columns


# ---- 2. the sweeps against the restatement ----------------------------------------------------------------------------------------------
def _seeds(K, B, nx, nu, kind='xu'):
    rng = np.random.default_rng(23)
    gx, gu = rng.standard_normal((K + 1, B, nx)), rng.standard_normal((K, B, nu))
    return (gx if 'x' in kind else None), (gu if 'u' in kind else None)


def _ref_entries(tape, b, nx, nu):
    """Instance b of a device tape (BatchProblem.rollout_tape per step) in the form of tests/rollout_ref.py."""
    out = []
    for e in tape:
        xr = e['step'][b, nx + nu:]
        out.append(dict(x=e['x'][b], z=e['z'][b], y=e['y'][b], x0=e['step'][b, :nx], um1=e['step'][b, nx:nx + nu],
                        xref=xr.reshape(-1, nx) if xr.size > nx else xr, solved=bool(e['status'][b] == SOLVED)))
    return out


def _held_to_the_restatement(C, draws, gx, gu, got, names, Ap=None, Bp=None, tol=TOL):
    """Every instance of a swept controller (draws: its (kw, attrs) per instance) against bounds_ref.sweep on the device's own tape."""
    K = gu.shape[0] if gu is not None else gx.shape[0] - 1
    tape = [C.prob.rollout_tape(k) for k in range(K)]
    D, E, cs, _ = C.prob.scaling()
    errs = {}
    for b, (kw, attrs) in enumerate(draws):
        ref = br.sweep(kw, attrs, _ref_entries(tape, b, C.nx, C.nu), D[b], E[b], cs[b], None if gx is None else gx[:, b], None if gu is None else gu[:, b],
                       Ap=None if Ap is None else Ap[b], Bp=None if Bp is None else Bp[b])
        assert np.array_equal(got['status'][:, b], ref['status']) and got['n_factor'][b] == ref['n_factor'], (b, got['status'][:, b], got['n_factor'][b])
        for k in names:
            v = got[k][:, b] if k in ('lam', 'xref') else got[k][b]
            errs[k] = max(errs.get(k, 0.0), _rel(v, ref[k]))
    return errs, np.array([e['status'] for e in tape])


@pytest.mark.parametrize('name', sorted({n for n, _ in bc.ROLLOUT}))
def test_the_state_feedback_sweep_is_the_restatement(name):
    """The listed seeds of an existing loop, on the forward tests/test_gpu_rollout.py shares (plant given, disturbed)."""
    f = rd.forward(name, True, True)
    Kb, c = f['Kb'], rc.CASES[name]
    gx, gu = _seeds(c['K'], Kb.B, c['nx'], c['nu'])
    got = Kb.rollout_adjoint(g_x=gx, g_u=gu, want=CHAIN + MODEL + BOUNDS)
    assert np.all(got['status'] == 1) and np.all(got['n_weak'] == 0)
    D, E, cs = f['scaling']
    errs, big = {}, 0.0
    for seed in (s for n, s in bc.ROLLOUT if n == name):
        b = c['seeds'].index(seed)
        kw, attrs = rc.draw(name, seed)
        ref = br.sweep(kw, attrs, rd.ref_tape(f, name, b), D[b], E[b], cs[b], gx[:, b], gu[:, b], Ap=f['io']['Ap'][b], Bp=f['io']['Bp'][b])
        for k in BOUNDS + MODEL:
            errs[k] = max(errs.get(k, 0.0), _rel(got[k][b], ref[k]))
        big = max(big, max(np.abs(ref[k]).max() for k in BOUNDS))
    print('BOUNDS_SWEEP %s: %s' % (name, ' '.join('%s=%.1e' % kv for kv in errs.items())))
    assert max(errs.values()) <= TOL, (name, errs)
    assert big > 1e-6, name


def _fresh_loop(name, B=2, **over):
    """B copies of a loop's instance as a BatchMPCController, set up and solved at EPS; ``over`` replaces constructor arguments."""
    from pympc_amd import BatchMPCController
    args = bc.loop_batch_kwargs(name, B, eps_abs=EPS, eps_rel=EPS, max_iter=400000)
    args.update(over)
    K = BatchMPCController(**args)
    K.setup()
    return K


@pytest.mark.parametrize('name', sorted(bc.LOOPS))
def test_the_new_loops_sweep_is_the_restatement(name):
    c = bc.LOOPS[name]
    C = _fresh_loop(name)
    tr = C.rollout(c['K'])
    assert np.all(tr['status'] == SOLVED)
    gx, gu = _seeds(c['K'], C.B, c['nx'], c['nu'])
    got = C.rollout_adjoint(g_x=gx, g_u=gu, want=CHAIN + MODEL + BOUNDS)
    assert np.all(got['n_weak'] == 0)
    errs, _ = _held_to_the_restatement(C, [bc.loop(name)] * C.B, gx, gu, got, CHAIN + MODEL + BOUNDS)
    print('BOUNDS_SWEEP %s: %s' % (name, ' '.join('%s=%.1e' % kv for kv in errs.items())))
    assert max(errs.values()) <= TOL, (name, errs)
    if name == 'xbox_soft':
        assert np.abs(got['xmin']).max() > 1e-6 and np.abs(got['xmax']).max() > 1e-6
    if name == 'ubox_tight':
        assert np.abs(got['umin']).max() > 1e-6 and np.abs(got['umax']).max() > 1e-6


def test_the_output_feedback_sweep_is_the_restatement():
    name = ec.FIRST
    f = rd.forward(name, True, True, est=True)
    Kb, c, ny = f['Kb'], rc.CASES[name], ec.ny_of(name)
    K, B = c['K'], Kb.B
    rng = np.random.default_rng(23)
    g = dict(x=rng.standard_normal((K + 1, B, c['nx'])), xh=rng.standard_normal((K + 1, B, c['nx'])), u=rng.standard_normal((K, B, c['nu'])), y=rng.standard_normal((K, B, ny)))
    names = ('lam', 'eta', 'uminus1', 'C', 'L', 'Ad') + BOUNDS
    got = Kb.rollout_adjoint(g_x=g['x'], g_u=g['u'], g_xhat=g['xh'], g_y=g['y'], want=names)
    plain = Kb.rollout_adjoint(g_x=g['x'], g_u=g['u'], g_xhat=g['xh'], g_y=g['y'], want=names[:6])
    for k in names[:6]:
        assert np.array_equal(got[k], plain[k]), k               # (mpcqp_rollout_adjoint_est: asking for bounds changes no bit of it)
    assert np.all(got['status'] == 1) and np.all(got['n_weak'] == 0)
    D, E, cs = f['scaling']
    io, errs, big = f['io'], {}, 0.0
    for b, seed in enumerate(f['seeds']):
        kw, attrs = rc.draw(name, seed)
        ref = br.sweep_est(kw, attrs, rd.ref_tape(f, name, b, est=True), D[b], E[b], cs[b], io['e']['C'][b], io['e']['L'][b], G_x=g['x'][:, b], G_xh=g['xh'][:, b],
                           G_u=g['u'][:, b], G_y=g['y'][:, b], Ap=io['Ap'][b], Bp=io['Bp'][b])
        for k in names:
            v = got[k][:, b] if k in ('lam', 'eta') else got[k][b]
            errs[k] = max(errs.get(k, 0.0), _rel(v, ref[k]))
        big = max(big, max(np.abs(ref[k]).max() for k in BOUNDS))
    print('BOUNDS_SWEEP_EST %s: %s' % (name, ' '.join('%s=%.1e' % kv for kv in errs.items())))
    assert max(errs.values()) <= TOL, errs
    assert big > 1e-6


@pytest.mark.parametrize('name', ('first', 'xbox_soft', 'hard_state'))
def test_one_step_with_no_state_seed_is_the_single_solve_call(name):
    K = rd.ctrl(name) if name in rc.CASES else _fresh_loop(name)
    g = np.random.default_rng(3).standard_normal((K.B, K.nu))
    one = K.adjoint(g_u0=g, want=CHAINED + BOUNDS)
    assert np.all(one['status'] == 1)
    K.rollout(1)
    got = K.rollout_adjoint(g_u=g[None], want=CHAIN + BOUNDS)
    for k in BOUNDS + ('uminus1',):
        assert _rel(got[k], one[k]) <= 1e-12, (name, k, _rel(got[k], one[k]))
    assert _rel(got['lam'][0], one['x0']) <= 1e-12 and np.all(got['n_factor'] == 1)
    assert max(np.abs(one[k]).max() for k in BOUNDS) > 1e-6


# ---- 3. end to end: central differences of run() itself ---------------------------------------------------------------------------------
def test_the_sweep_against_central_differences_of_the_device_loop():
    """L = sum <Gx[k], x_k> + sum <Gu[k], u_k> of run(K) on fresh controllers, in one direction of each of the six bounds, on the loops the
    oracle's central differences use (tests/bounds_cases.FD_LOOPS): method, step h = 1e-4 and bound of
    tests/test_gpu_rollout.py::test_the_sweep_against_central_differences_of_the_device_loop."""
    h, seen = 1e-4, {k: 0.0 for k in BOUNDS}
    rng = np.random.default_rng(29)
    for name in bc.FD_LOOPS:
        c = bc.LOOPS[name]
        K, B = c['K'], 1
        gx, gu = _seeds(K, B, c['nx'], c['nu'])
        C = _fresh_loop(name, B)
        C.rollout(K)
        got = C.rollout_adjoint(g_x=gx, g_u=gu, want=BOUNDS)
        assert np.all(got['status'] == 1) and np.all(got['n_weak'] == 0)
        base = bc.loop_batch_kwargs(name, B)

        def loss(over):
            tr = _fresh_loop(name, B, **over).run(K)
            return (gx * tr['x']).sum(axis=(0, 2)) + (gu * tr['u']).sum(axis=(0, 2))

        for field in BOUNDS:
            d = rng.standard_normal(base[field].shape)
            d /= np.sqrt((d * d).sum(axis=1))[:, None]
            fd = (loss({field: base[field] + h * d}) - loss({field: base[field] - h * d})) / (2 * h)
            an = (got[field] * d).sum(axis=1)
            err = np.abs(an - fd).max()
            print('BOUNDS_FD %s d/d%s: |grad.d - FD|_inf = %.3e, |FD|_inf = %.3e' % (name, field, err, np.abs(fd).max()))
            assert err <= FD_TOL * max(1.0, np.abs(fd).max()), (name, field, err, an, fd)
            seen[field] = max(seen[field], np.abs(fd).max())
    assert all(v > 1e-3 for v in seen.values()), seen            # (every bound is held by a difference that is not in the noise)


# ---- 4. bits ----------------------------------------------------------------------------------------------------------------------------
def _io(cls, **fields):
    s = cls()
    s.struct_size = C.sizeof(cls)
    for k, v in fields.items():
        setattr(s, k, v if isinstance(v, int) else v.ctypes.data)
    return s


def test_bounds_change_no_other_bit_and_null_is_the_older_call():
    from pympc_amd import _lib
    Ka, Kb = rd.ctrl(rc.FIRST), rd.ctrl(rc.FIRST)
    before = ac.snapshot(Ka.prob)
    assert ac.same(before, ac.snapshot(Kb.prob))
    B, bp = Ka.B, Ka.prob
    g, gu = np.random.default_rng(3).standard_normal((B, bp.n)), np.ones((B, bp.nu))
    older = CHAINED + RAW + MODEL
    plain = Kb.prob.adjoint(g_w=g, g_u0=gu, want=older)
    one = bp.adjoint(g_w=g, g_u0=gu, want=older + BOUNDS)
    assert np.all(bp.adjoint_info()[2] == 1)
    for k in older:
        assert np.array_equal(plain[k], one[k]), k
    only = bp.adjoint(g_w=g, g_u0=gu, want=BOUNDS)            # (nothing of mpcqp_adjoint_io or mpcqp_adjoint_model_io asked for)
    two = bp.adjoint(g_w=g, g_u0=gu, want=BOUNDS)
    s1, s2 = (bp.adjoint(g_w=g, g_u0=gu, want=BOUNDS + ('Ad',), batch_sum=True) for _ in range(2))
    for k in BOUNDS:
        assert np.array_equal(one[k], only[k]) and np.array_equal(one[k], two[k]) and np.array_equal(s1[k], s2[k]), k
        assert s1[k].shape == (1,) + one[k].shape[1:]
        assert np.all(np.abs(s1[k][0] - one[k].sum(axis=0)) <= B * 1.2e-16 * 4 * np.abs(one[k]).sum(axis=0)), k
    assert max(np.abs(one[k]).max() for k in BOUNDS) > 1e-6
    # bo == NULL: mpcqp_adjoint_model, bit for bit
    L, h = bp._L, bp._h
    outs = [(np.zeros((B, bp.nx)), np.zeros((B, bp.nx, bp.nx))) for _ in range(2)]
    for (x0, dA), call in zip(outs, (lambda io, mo: L.mpcqp_adjoint_model(h, C.byref(io), C.byref(mo)),
                                    lambda io, mo: L.mpcqp_adjoint_bounds(h, C.byref(io), C.byref(mo), None))):
        assert call(_io(_lib.AdjointIO, g_u0=gu, d_x0=x0), _io(_lib.AdjointModelIO, d_Ad=dA)) == 0
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and np.any(outs[0][1] != 0.0)
    # the same for the sweep: bounds change no other bit, reuse on and off agree, NULL is mpcqp_rollout_adjoint
    K = 3
    ta, tb = Ka.rollout(K), Kb.rollout(K)
    gx, gu3 = _seeds(K, B, bp.nx, bp.nu)
    p = Kb.rollout_adjoint(g_x=gx, g_u=gu3, want=CHAIN + MODEL)
    a = Ka.rollout_adjoint(g_x=gx, g_u=gu3, want=CHAIN + MODEL + BOUNDS)
    a2 = Ka.rollout_adjoint(g_x=gx, g_u=gu3, want=BOUNDS)
    nr = Ka.rollout_adjoint(g_x=gx, g_u=gu3, want=CHAIN + MODEL + BOUNDS, no_reuse=True)
    t1, t2 = (Ka.rollout_adjoint(g_x=gx, g_u=gu3, want=BOUNDS, batch_sum=True) for _ in range(2))
    assert np.all(a['status'] == 1)
    for k in CHAIN + MODEL:
        assert np.array_equal(p[k], a[k]) and np.array_equal(a[k], nr[k]), k
    for k in BOUNDS:
        assert np.array_equal(a[k], a2[k]) and np.array_equal(a[k], nr[k]) and np.array_equal(t1[k], t2[k]), k
        assert np.all(np.abs(t1[k][0] - a[k].sum(axis=0)) <= B * 1.2e-16 * 4 * np.abs(a[k]).sum(axis=0)), k
    assert max(np.abs(a[k]).max() for k in BOUNDS) > 1e-6
    outs = [(np.zeros((K + 1, B, bp.nx)), np.zeros((B, bp.nx, bp.nx))) for _ in range(2)]
    for (lam, dA), call in zip(outs, (lambda io, mo: L.mpcqp_rollout_adjoint(h, C.byref(io), C.byref(mo)),
                                     lambda io, mo: L.mpcqp_rollout_adjoint_bounds(h, C.byref(io), None, C.byref(mo), None))):
        assert call(_io(_lib.RolloutAdjointIO, G_x=gx, G_u=gu3, lam=lam), _io(_lib.AdjointModelIO, d_Ad=dA)) == 0
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][0], a['lam'])
    # a solve after the calls is the solve without them
    assert ac.same(ac.snapshot(Ka.prob), ac.snapshot(Kb.prob))
    x1 = np.array(rc.batch_kwargs(rc.FIRST)['x0']) * 0.9
    for Kc in (Ka, Kb):
        Kc.update(x1)
    assert ac.same(ac.snapshot(Ka.prob), ac.snapshot(Kb.prob))
    ra, rb = Ka.run(2), Kb.run(2)
    for k in ('x', 'u', 'status', 'iter'):
        assert np.array_equal(ra[k], rb[k]), k


# ---- 5. zeros and refusals --------------------------------------------------------------------------------------------------------------
def test_an_unsolved_instance_gets_zeros_and_adds_nothing_to_the_sum():
    name, bad = ac.INFEASIBLE
    s = ac.CASES[name]['seeds']
    Ka, Kb = ac.case_batch(name, (s[0], s[1], bad, s[2])), ac.case_batch(name, (s[0], s[1], s[2]))
    assert Ka.status() == ['solved', 'solved', 'primal infeasible', 'solved'], Ka.status()
    ga = np.random.default_rng(7).standard_normal((4, Ka.prob.n))
    ra, rb = Ka.prob.adjoint(g_w=ga, want=BOUNDS), Kb.prob.adjoint(g_w=ga[[0, 1, 3]], want=BOUNDS)
    assert list(Ka.prob.adjoint_info()[2]) == [1, 1, 0, 1]
    sa, sb = Ka.prob.adjoint(g_w=ga, want=BOUNDS, batch_sum=True), Kb.prob.adjoint(g_w=ga[[0, 1, 3]], want=BOUNDS, batch_sum=True)
    for k in BOUNDS:
        assert np.all(ra[k][2] == 0.0) and np.all(np.isfinite(ra[k])), k
        assert np.array_equal(ra[k][[0, 1, 3]], rb[k]), k
        assert np.all(np.abs(sa[k] - sb[k]) <= 4 * 1.2e-16 * 4 * np.abs(rb[k]).sum(axis=0)), k
    assert max(np.abs(rb[k]).max() for k in BOUNDS) > 1e-6


def test_a_failed_step_in_the_middle_of_a_tape_adds_nothing():
    """The failed entry of tests/test_gpu_rollout.py::test_a_failed_step_in_the_middle_of_a_tape: the restatement, which skips it, holds."""
    name = 'hard'
    c = rc.CASES[name]
    K = c['K']
    x1 = rd.ctrl(name).run(1)['x'][1]
    w = np.zeros((K, len(c['seeds']), c['nx'])); w[0, 0, 0] = 6.0 - x1[0, 0]      # x_1[0] = 6 against a box of 4
    Cc = rd.ctrl(name)
    Cc.rollout(K, w=w)
    gx, gu = _seeds(K, Cc.B, c['nx'], c['nu'])
    got = Cc.rollout_adjoint(g_x=gx, g_u=gu, want=CHAIN + BOUNDS)
    errs, taped = _held_to_the_restatement(Cc, [rc.draw(name, s) for s in c['seeds']], gx, gu, got, CHAIN + BOUNDS)
    assert taped[1, 0] != SOLVED and np.all(np.delete(taped[:, 0], 1) == SOLVED) and np.all(taped[:, 1:] == SOLVED), taped
    assert got['status'][1, 0] == 0 and max(errs.values()) <= TOL, errs


def test_infinite_bounds_get_exact_zeros():
    kw = ac.golden('quadcopter_nodu')
    K = ac.solved(kw)
    bp = K.prob.batch_problem
    got = bp.adjoint(g_w=np.random.default_rng(7).standard_normal((1, bp.n)), want=BOUNDS)
    assert bp.adjoint_info()[2][0] == 1
    assert np.all(got['Dumin'] == 0.0) and np.all(got['Dumax'] == 0.0)
    assert np.all(got['xmin'][0][~np.isfinite(kw['xmin'])] == 0.0) and np.all(got['xmax'][0][~np.isfinite(kw['xmax'])] == 0.0)
    assert max(np.abs(got[k]).max() for k in BOUNDS) > 1e-6            # (the finite ones are active)


def test_refusals():
    from pympc_amd import _lib
    from pympc_amd.solver import DeviceProblem
    from polish_ref import golden_qp
    # raw-vector mode: the bounds are l, u themselves
    P, q, A, l, u = golden_qp(util.load_golden('random_12_4_30_b'))
    prob = DeviceProblem()
    prob.setup(P, q, A, l, u, eps_abs=EPS, eps_rel=EPS, max_iter=400000)
    assert prob.solve().info.status == 'solved'
    raw = prob.batch_problem
    for k in BOUNDS:
        with pytest.raises(RuntimeError, match=r'\(-5\)'):
            raw.adjoint(g_u0=np.ones((1, raw.nu)), want=(k,))
    assert np.any(raw.adjoint(g_u0=np.ones((1, raw.nu)), want=RAW)['l'] != 0.0)
    # struct_size, nothing asked for, an unknown name
    Kc = _fresh_loop('ubox_tight', 1)
    bp = Kc.prob
    gu, dst, x0 = np.ones((1, bp.nu)), np.zeros((1, bp.nu)), np.zeros((1, bp.nx))
    io, bo = _io(_lib.AdjointIO, g_u0=gu), _io(_lib.AdjointBoundsIO, d_umax=dst)
    call = lambda: bp._L.mpcqp_adjoint_bounds(bp._h, C.byref(io), None, C.byref(bo))
    assert call() == 0 and np.any(dst != 0.0)
    bo.struct_size -= 8
    assert call() == -1                                         # MPCQP_ERR_ARG
    bo.struct_size += 8
    bo.batch_sum = 2
    assert call() == -1
    bo.batch_sum = 0
    bo.d_umax = None
    assert call() == -1                                         # nothing asked for in any struct
    io.d_x0 = x0.ctypes.data
    assert call() == 0 and np.any(x0 != 0.0)                    # (an output of io is enough)
    with pytest.raises(TypeError):
        bp.adjoint(g_u0=gu, want=('umax', 'vmax'))
    # the sweep: no tape, then a stale one
    g2 = np.ones((2, 1, bp.nu))
    ro = _io(_lib.RolloutAdjointIO, G_u=g2)
    bo = _io(_lib.AdjointBoundsIO, d_umax=dst)
    sweep = lambda: bp._L.mpcqp_rollout_adjoint_bounds(bp._h, C.byref(ro), None, None, C.byref(bo))
    assert sweep() == -5                                        # MPCQP_ERR_STATE: no tape
    Kc.rollout(2)
    assert sweep() == 0
    bo.d_umax = None
    assert sweep() == -1                                        # nothing asked for
    bo.d_umax = dst.ctypes.data
    bo.struct_size += 8
    assert sweep() == -1
    bo.struct_size -= 8
    Kc.update_model(umax=Kc.umax, solve=False)
    assert sweep() == -5                                        # the tape's model was replaced
    with pytest.raises(RuntimeError, match=r'\(-5\)'):
        Kc.rollout_adjoint(g_u=np.ones((2, 1, bp.nu)), want=('umax',))
    with pytest.raises(TypeError):
        Kc.rollout_adjoint(g_u=np.ones((2, 1, bp.nu)), want=('vmax',))


# ---- 6. torch ---------------------------------------------------------------------------------------------------------------------------
def _step_case(B):
    kw = am.full_kwargs(bc.loop('ubox_tight')[0])
    nx, nu = kw['Bd'].shape
    rng = np.random.default_rng(11)
    x = np.stack([kw['x0']] * B) + 0.001 * rng.standard_normal((B, nx))
    um1 = np.stack([kw['uminus1']] * B) + 0.001 * rng.standard_normal((B, nu))
    return kw, x, um1, rng.standard_normal((B, nu))


def _u_of(kw, B, x, um1, **bounds):
    """A fresh controller, the bounds put under it, one cold step: both ends of a difference alike (and what mpc_step's forward does)."""
    K = ac.copies(kw, B); K.setup(solve=False)
    K.update_model(solve=False, **bounds)
    return np.array(K.step(x, um1))


def test_mpc_step_bound_gradients_against_central_differences():
    """Every entry of the six bounds, h = 1e-5, device solves at eps 1e-9 through update_model; bound 1e-4 max(1, |fd|_inf): the method of
    tests/test_gpu_adjoint_model.py::test_mpc_step_parameter_gradients_against_central_differences."""
    import torch
    from pympc_amd.torch_layer import mpc_step
    B = 2
    kw, x, um1, w = _step_case(B)
    dev = torch.device('cuda:0')
    base = {k: np.stack([kw[k]] * B) for k in BOUNDS}
    bounds = {k: torch.tensor(v, dtype=torch.float64, device=dev, requires_grad=True) for k, v in base.items()}
    K = ac.copies(kw, B); K.setup(solve=False)
    u = mpc_step(K, torch.tensor(x, device=dev), torch.tensor(um1, device=dev), bounds=bounds)
    assert np.array_equal(u.detach().cpu().numpy(), _u_of(kw, B, x, um1, **base))
    (u * torch.tensor(w, device=dev)).sum().backward()
    _, nweak, status = K.prob.adjoint_info()
    assert np.all(status == 1) and np.all(nweak == 0), (status, nweak)
    h, seen = 1e-5, 0.0
    for k in BOUNDS:
        grad = bounds[k].grad
        assert grad is not None and tuple(grad.shape) == base[k].shape, k
        grad = grad.cpu().numpy()
        fd = np.zeros_like(base[k])
        for j in range(base[k].shape[1]):
            ends = []
            for s in (+h, -h):
                M = base[k].copy(); M[:, j] += s
                ends.append(_u_of(kw, B, x, um1, **dict(base, **{k: M})))
            fd[:, j] = ((ends[0] - ends[1]) * w).sum(axis=1) / (2 * h)
        err, big = np.abs(grad - fd).max(), np.abs(fd).max()
        print('BOUNDS_TORCH_FD d/d%s: |grad - FD|_inf = %.3e, |FD|_inf = %.3e' % (k, err, big))
        assert err <= 1e-4 * max(1.0, big), (k, err)
        seen = max(seen, big)
    assert seen > 1e-3


def test_mpc_step_unbatched_bounds_get_the_batch_sum_and_none_changes_nothing():
    import torch
    from pympc_amd.torch_layer import mpc_step
    B = 5
    kw, x, um1, w = _step_case(B)
    dev = torch.device('cuda:0')
    tx, tu, tw = torch.tensor(x, device=dev), torch.tensor(um1, device=dev), torch.tensor(w, device=dev)
    names, grads = ('umin', 'umax', 'Dumax'), []
    for batched in (True, False):
        bounds = {k: torch.tensor(np.stack([kw[k]] * B) if batched else kw[k], dtype=torch.float64, device=dev, requires_grad=True) for k in names}
        K = ac.copies(kw, B); K.setup(solve=False)
        u = mpc_step(K, tx, tu, bounds=bounds, params=dict(Ad=torch.tensor(kw['Ad'], device=dev)))
        (u * tw).sum().backward()
        grads.append({k: p.grad.cpu().numpy() for k, p in bounds.items()})
    for k in names:
        assert grads[1][k].shape == kw[k].shape, k
        assert np.all(np.abs(grads[1][k] - grads[0][k].sum(axis=0)) <= B * 1.2e-16 * 4 * np.abs(grads[0][k]).sum(axis=0)), k
    assert max(np.abs(grads[1][k]).max() for k in names) > 1e-6
    res = []
    for extra in ({}, dict(bounds=None)):                       # bounds=None: the layer as it was
        K = ac.copies(kw, B); K.setup(solve=False)
        t = tx.clone().requires_grad_(True)
        u = mpc_step(K, t, tu, **extra)
        (u * tw).sum().backward()
        res.append((u.detach().cpu().numpy(), t.grad.cpu().numpy()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    with pytest.raises(TypeError):
        mpc_step(K, tx, tu, params=dict(xmin=tx))                # params keeps refusing the bounds
    with pytest.raises(TypeError):
        mpc_step(K, tx, tu, bounds=dict(Ad=tx))


@pytest.mark.parametrize('est', (False, True), ids=('mpc_rollout', 'mpc_rollout_est'))
def test_the_rollout_layers_with_bounds(est):
    """The layer's bound gradients are the one sweep's with the seeds the loss implies (the method of
    tests/test_gpu_rollout.py::test_mpc_rollout_is_one_sweep_with_the_matching_seeds), unbatched ones its batch sum -- and they agree with a
    central difference of the layer's own forward in a direction of all the bounds at once (h = 1e-4, FD_TOL)."""
    import torch
    from pympc_amd.torch_layer import mpc_rollout, mpc_rollout_est
    name, B = 'ubox_tight', 2
    c = bc.LOOPS[name]
    K, nx, nu = c['K'], c['nx'], c['nu']
    dev = torch.device('cuda:0')
    t = lambda a, g=False: torch.tensor(np.asarray(a, dtype=float), dtype=torch.float64, device=dev, requires_grad=g)
    base = bc.loop_batch_kwargs(name, B)
    gx, gu = _seeds(K, B, nx, nu)
    e = None
    if est:
        from pympc_amd.kalman import kalman_design_simple
        Cm = np.random.default_rng(900).standard_normal((2, nx))
        Lg = kalman_design_simple(base['Ad'][0], None, Cm, None, 0.01 * np.eye(nx), 0.01 * np.eye(2), 'filter')[0]
        e = dict(C=t(Cm), L=t(Lg), x0=t(base['x0'] + 0.01))

    def run(bounds):
        Kc = _fresh_loop(name, B)
        if est:
            X, XH, Y, U = mpc_rollout_est(Kc, e['x0'], t(base['x0']), K, e['C'], e['L'], bounds=bounds)
        else:
            X, U = mpc_rollout(Kc, t(base['x0']), K, bounds=bounds)
        return Kc, X, U, (t(gx) * X).sum() + (t(gu) * U).sum()

    batched = {k: t(base[k], True) for k in BOUNDS}
    Kc, X, U, loss = run(batched)
    grads = dict(zip(BOUNDS, torch.autograd.grad(loss, [batched[k] for k in BOUNDS])))
    ref = Kc.prob.rollout_adjoint(g_x=gx, g_u=gu, want=BOUNDS)
    assert np.all(Kc.prob.rollout_info()[2] == 1) and np.all(Kc.prob.rollout_info()[1] == 0)
    for k in BOUNDS:
        assert grads[k].is_cuda and tuple(grads[k].shape) == base[k].shape and _rel(grads[k].cpu().numpy(), ref[k]) <= 1e-13, k
    shared = {k: t(base[k][0], True) for k in BOUNDS}
    Ks, _, _, loss_s = run(shared)
    gs = dict(zip(BOUNDS, torch.autograd.grad(loss_s, [shared[k] for k in BOUNDS])))
    tot = Ks.prob.rollout_adjoint(g_x=t(gx), g_u=t(gu), want=BOUNDS, batch_sum=True)
    for k in BOUNDS:
        assert tuple(gs[k].shape) == base[k].shape[1:] and torch.equal(gs[k], tot[k][0]), k
        assert np.all(np.abs(gs[k].cpu().numpy() - ref[k].sum(axis=0)) <= B * 1.2e-16 * 4 * np.abs(ref[k]).sum(axis=0)), k
    rng = np.random.default_rng(31)
    d = {k: rng.standard_normal(base[k].shape) for k in BOUNDS}
    h = 1e-4
    ends = [run({k: t(base[k] + s * h * d[k]) for k in BOUNDS})[3].item() for s in (1.0, -1.0)]
    fd, an = (ends[0] - ends[1]) / (2 * h), sum(float((grads[k].cpu().numpy() * d[k]).sum()) for k in BOUNDS)
    print('BOUNDS_TORCH_FD %s: grad.d %+.6e fd %+.6e' % ('mpc_rollout_est' if est else 'mpc_rollout', an, fd))
    assert abs(an - fd) <= FD_TOL * max(1.0, abs(fd)), (an, fd)
    assert abs(fd) > 1e-2


# ---- 7. the example ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_learn_constraints_example_descends():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'learn_constraints_through_mpc.py'), '--iters', '8', '--batch', '64'],
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout)
    loss = [float(v) for v in re.findall(r'^iteration +\d+: loss ([0-9.e+-]+)', r.stdout, flags=re.M)]
    assert len(loss) == 9 and loss[-1] < loss[0], loss
    for k in ('umax', 'Dumax'):
        d = re.search(k + r' ([0-9.e+-]+) -> ([0-9.e+-]+)', r.stdout)
        assert d and float(d.group(2)) < float(d.group(1)), r.stdout[-500:]
    active = re.search(r'expert: (\d+) of', r.stdout)
    assert active and int(active.group(1)) > 0
