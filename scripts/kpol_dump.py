#!/usr/bin/env python3
"""Everything k_polish, k_adjoint and the taped rollouts with their reverse sweeps compute, on the smallest cases that reach each of their
code paths, written into one npz -- to compare two builds of the library bit for bit (a refactoring of mpcqp_kpol.h / mpcqp_polish.h /
mpcqp_adjoint.h, or of the host side of mpcqp.hip, must not move a single bit):

    python scripts/with_lib.py <parent.so> scripts/kpol_dump.py a.npz
    python scripts/kpol_dump.py b.npz
    python scripts/kpol_dump.py --compare a.npz b.npz        # exit status 1 if any array differs (float64 compared as uint64)

Per case: after polish() the polished x, y, the iterate x, z, y, status_polish, obj_val / pri_res / dua_res; every output of
adjoint(g_u0=..., want = all fourteen names) with and without batch_sum; every matrix of gains(); adjoint_info().  Cases: six golden
fixtures, the first seed of six shapes of tests/adjoint_cases.py, a batch with an unsolved instance, a raw-vector handle (want q, l, u),
an MPCController with polish=True stepped through update() (mpcqp_step_host), adjoint() right after BatchMPCController.step().
Rollouts (tests/rollout_cases.py, tests/rollout_est_cases.py, the cases' own instances and step counts, seeds from default_rng(3)): per
case of ROLLOUT, with the controller's model as the plant and with a plant of its own, the trajectory, the first and the last tape entry,
every output of rollout_adjoint plain, with batch_sum and with no_reuse, and rollout_info() behind each; per case of ROLLOUT_EST the same
of rollout_est with its four seeds (plain and batch_sum), then the sweep of g_x, g_u alone on that tape; and one handle taken through
step() -> adjoint() -> rollout -> rollout_adjoint -> rollout_est -> rollout_adjoint (the moved u_{-1}, a tape replaced by one of the other kind)."""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

EPS = 1e-9
GOLDEN = ('cart_pole', 'cart_pole_nc1', 'point_mass_hard', 'small_mimo', 'random_5_3_8', 'quadcopter_nodu')
SHAPES = ('nb16_nu6', 'nb16_nu7_hard', 'nb32_nu9_held', 'nb64_nu10_held', 'nb128_nu5', 'long200_nu2')
CHAINED = ('x0', 'uminus1', 'xref', 'uref')
RAW = ('q', 'l', 'u')
MODEL = ('Ad', 'Bd', 'Qx', 'QxN', 'Qu', 'QDu', 'eps_feas')
ROLLOUT = ('first', 'first_tvref', 'held', 'nb32_soft', 'nb64', 'nb128')
ROLLOUT_EST = ('first', 'held', 'nb32_soft')
SWEEP = ('lam', 'uminus1', 'uref', 'xref', 'Ap', 'Bp') + MODEL
SWEEP_EST = SWEEP + ('eta', 'C', 'L', 'v', 'Ae', 'Be')


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    for k in sorted(set(A.files) & set(B.files)):
        x, y = A[k], B[k]
        same = x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x,
                                                                          y.view(np.uint64) if y.dtype == np.float64 else y)
        if not same:
            bad.append(k)
    print('KPOL_COMPARE %d arrays, %d differ%s' % (len(A.files), len(bad), ': ' + ' '.join(bad) if bad else ''))
    print('KPOL_ARRAYS ' + ' '.join(sorted(A.files)))
    return 1 if bad else 0


def dump_polish(out, tag, bp):
    """polish() on the handle's last solve: the polished point, the iterate it replaces, its status and figures."""
    bp.polish()
    st = bp.polish_status()
    x, y = bp.solution()[:2]
    xi, zi, yi = bp.iterate_state()[:3]
    infos = bp.infos()
    out.update({tag + '/pol_x': np.array(x), tag + '/pol_y': np.array(y), tag + '/it_x': np.array(xi), tag + '/it_z': np.array(zi),
                tag + '/it_y': np.array(yi), tag + '/status_polish': np.array(st),
                tag + '/obj_pri_dua': np.array([[i.obj_val, i.pri_res, i.dua_res] for i in infos])})


def dump_adjoint(out, tag, bp, want=CHAINED + RAW + MODEL, gains=True):
    g = np.random.default_rng(3).standard_normal((bp.batch, bp.nu))
    for bs in (False, True) if any(k in MODEL for k in want) else (False,):
        res = bp.adjoint(g_u0=g, want=want, batch_sum=bs)
        out.update({'%s/adj%d_%s' % (tag, bs, k): np.array(v) for k, v in res.items()})
        out['%s/adj%d_info' % (tag, bs)] = np.stack(bp.adjoint_info())
    if gains:
        out.update({'%s/K_%s' % (tag, k): np.array(v) for k, v in bp.gains().items()})
        out[tag + '/K_info'] = np.stack(bp.adjoint_info())


def put(out, tag, d):
    out.update({'%s/%s' % (tag, k): np.array(v) for k, v in d.items()})


def dump_sweep(out, tag, bp, **kw):
    """One rollout_adjoint call: every gradient it was asked for, and rollout_info() behind it."""
    put(out, tag, bp.rollout_adjoint(**kw))
    put(out, tag + '_info', dict(zip(('n_active', 'n_weak', 'status', 'n_factor'), bp.rollout_info())))


def dump_tape(out, tag, bp, K):
    for k in sorted({0, K - 1}):
        put(out, '%s/tape%d' % (tag, k), bp.rollout_tape(k))


def dump_rollout(out, name, ctrl):
    import rollout_cases as rc
    c = rc.CASES[name]
    K, B, nx, nu = c['K'], len(c['seeds']), c['nx'], c['nu']
    rng = np.random.default_rng(3)
    g = dict(g_x=rng.standard_normal((K + 1, B, nx)), g_u=rng.standard_normal((K, B, nu)))
    dA, dB = 0.02 * rng.standard_normal((B, nx, nx)), 0.02 * rng.standard_normal((B, nx, nu))
    xr = np.stack([rc.xref_traj(name, s) for s in c['seeds']], axis=1).reshape(K, B, -1) if c['tv'] else None
    for own in (0, 1):
        Kc = ctrl(rc.batch_kwargs(name))
        tag = 'rollout/%s/plant%d' % (name, own)
        put(out, tag, Kc.rollout(K, Ap=Kc.Ad + dA if own else None, Bp=Kc.Bd + dB if own else None, xref_traj=xr))
        dump_tape(out, tag, Kc.prob, K)
        for v, kw in (('adj', {}), ('adj_sum', dict(batch_sum=True)), ('adj_no_reuse', dict(no_reuse=True))):
            dump_sweep(out, '%s/%s' % (tag, v), Kc.prob, want=SWEEP, **dict(g, **kw))


def est_inputs(name, Kc):
    """(the estimator object of a case on controller Kc, its disturbances w, the four seeds of its sweep)"""
    import rollout_cases as rc
    import rollout_est_cases as ec
    from pympc_amd.kalman import BatchLinearStateEstimator
    c = rc.CASES[name]
    K, B, nx, ny = c['K'], Kc.B, c['nx'], ec.ny_of(name)
    e = ec.batch_estimator(name)
    rng = np.random.default_rng(3)
    g = dict(g_x=rng.standard_normal((K + 1, B, nx)), g_u=rng.standard_normal((K, B, c['nu'])), g_xhat=rng.standard_normal((K + 1, B, nx)),
             g_y=rng.standard_normal((K, B, ny)))
    return BatchLinearStateEstimator(Kc.x0, Kc.Ad, Kc.Bd, e['C'], e['L'], x_true=np.array(e['x_true0']), v=e['v']), e['w'], g


def dump_rollout_est(out, name, ctrl):
    import rollout_cases as rc
    import rollout_est_cases as ec
    K = rc.CASES[name]['K']
    Kc = ctrl(ec.batch_kwargs(name))
    est, w, g = est_inputs(name, Kc)
    tag = 'rollout_est/' + name
    put(out, tag, Kc.rollout_est(K, est, w=w))
    dump_tape(out, tag, Kc.prob, K)
    for bs in (False, True):
        dump_sweep(out, '%s/adj%d' % (tag, bs), Kc.prob, want=SWEEP_EST, batch_sum=bs, **g)
    dump_sweep(out, tag + '/adj_xu', Kc.prob, want=SWEEP_EST, g_x=g['g_x'], g_u=g['g_u'])


def dump_sequence(out, ctrl, name='first'):
    """One handle: step() -> adjoint() -> rollout -> rollout_adjoint -> rollout_est -> rollout_adjoint."""
    import rollout_cases as rc
    import rollout_est_cases as ec
    K = rc.CASES[name]['K']
    Kc = ctrl(ec.batch_kwargs(name))
    est, w, g = est_inputs(name, Kc)
    rng = np.random.default_rng(11)
    tag = 'sequence'
    out[tag + '/u'] = np.array(Kc.step(Kc.x0 + 0.01 * rng.standard_normal(Kc.x0.shape), Kc.uminus1 + 0.01 * rng.standard_normal(Kc.uminus1.shape)))
    dump_adjoint(out, tag, Kc.prob, want=CHAINED + MODEL, gains=False)
    put(out, tag + '/rollout', Kc.rollout(K, w=w))
    dump_tape(out, tag + '/rollout', Kc.prob, K)
    dump_sweep(out, tag + '/rollout/adj', Kc.prob, want=SWEEP, g_x=g['g_x'], g_u=g['g_u'])
    put(out, tag + '/rollout_est', Kc.rollout_est(K, est, w=w))
    dump_tape(out, tag + '/rollout_est', Kc.prob, K)
    dump_sweep(out, tag + '/rollout_est/adj', Kc.prob, want=SWEEP_EST, **g)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == '--compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2 or sys.argv[1].startswith('-'):
        sys.exit('usage: kpol_dump.py <out.npz> | kpol_dump.py --compare <a.npz> <b.npz>')
    import adjoint_cases as ac
    import adjoint_model_ref as am
    from util import golden_kwargs, load_golden, apply_attrs, KW, repeated
    from pympc_amd import MPCController, BatchMPCController
    out = {}

    def controller(kw, **settings):
        attrs = getattr(kw, 'attrs', {})
        kw = KW(kw); kw.attrs = attrs
        kw.update(eps_abs=EPS, eps_rel=EPS)
        K = apply_attrs(MPCController(**kw), kw)
        K.solver_settings = dict(max_iter=400000, **settings)
        K.setup()
        return K

    def ctrl(args):
        K = BatchMPCController(**dict(args, eps_abs=EPS, eps_rel=EPS, max_iter=400000))
        K.setup()
        return K

    def batch(name, seeds):
        return ctrl(ac.batch_kwargs(name, seeds))

    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for name in GOLDEN:                       # the adjoint first: it differentiates the solve, polish() then replaces the iterate
            bp = controller(golden_kwargs(load_golden(name))).prob.batch_problem
            dump_adjoint(out, name, bp)
            dump_polish(out, name, bp)
        for name in SHAPES:
            bp = batch(name, ac.CASES[name]['seeds'][:1]).prob
            dump_adjoint(out, name, bp)
            dump_polish(out, name, bp)
        name, bad = ac.INFEASIBLE                 # an unsolved instance among the columns: the "not computed" path
        s = ac.CASES[name]['seeds']
        K = batch(name, (s[0], s[1], bad, s[2]))
        assert K.status()[2] == 'primal infeasible', K.status()
        dump_adjoint(out, 'mixed', K.prob)
        dump_polish(out, 'mixed', K.prob)
        # raw-vector mode (chain = 0): only q, l, u
        from pympc_amd.solver import DeviceProblem
        from polish_ref import golden_qp
        P, q, A, l, u = golden_qp(load_golden('random_12_4_30_b'))
        prob = DeviceProblem()
        prob.setup(P, q, A, l, u, eps_abs=EPS, eps_rel=EPS, max_iter=400000)
        assert prob.solve().info.status == 'solved'
        bp = prob.batch_problem
        res = bp.adjoint(g_w=np.random.default_rng(5).standard_normal((1, bp.n)), want=RAW)
        out.update({'raw/adj_' + k: np.array(v) for k, v in res.items()})
        out['raw/adj_info'] = np.stack(bp.adjoint_info())
        dump_polish(out, 'raw', bp)
        # MPCController with polish=True through update(): k_polish's pub / done path under mpcqp_step_host
        kw = golden_kwargs(load_golden('cart_pole'))
        K = controller(kw, polish=True)
        kw = am.full_kwargs(kw)
        x = np.array(kw['x0'], dtype=float)
        us, sp = [], []
        for _ in range(4):
            u = K.output()
            x = np.asarray(kw['Ad']) @ x + np.asarray(kw['Bd']) @ u
            K.update(x, u)
            us.append(np.array(K.output(), dtype=float)); sp.append(int(K.res.info.status_polish))
        out['step_host/u'] = np.array(us); out['step_host/status_polish'] = np.array(sp)
        out['step_host/x'] = np.array(K.res.x, dtype=float); out['step_host/y'] = np.array(K.res.y, dtype=float)
        # adjoint() right after BatchMPCController.step(): the step data hold the applied input, the kernels read the copy with u_{-1} put back
        kw = am.full_kwargs(golden_kwargs(load_golden('small_mimo')))
        B = 3
        st = lambda k: np.stack([np.asarray(kw[k], dtype=float)] * B)
        K = BatchMPCController(**repeated(kw, B, eps_feas=kw.get('eps_feas', 1e6), eps_abs=EPS, eps_rel=EPS, max_iter=400000))
        K.setup(solve=False)
        rng = np.random.default_rng(11)
        out['after_step/u'] = np.array(K.step(st('x0') + 0.01 * rng.standard_normal((B, st('x0').shape[1])),
                                              st('uminus1') + 0.01 * rng.standard_normal((B, st('uminus1').shape[1]))))
        dump_adjoint(out, 'after_step', K.prob)
        for name in ROLLOUT:
            dump_rollout(out, name, ctrl)
        for name in ROLLOUT_EST:
            dump_rollout_est(out, name, ctrl)
        dump_sequence(out, ctrl)
    np.savez(sys.argv[1], **out)
    print('KPOL_DUMP %d arrays -> %s' % (len(out), sys.argv[1]))


if __name__ == '__main__':
    main()
