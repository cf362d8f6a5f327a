"""The affine term of the prediction model, x_{k+1} = Ad x_k + Bd u_k + d_k (include_ext4/mpcqp_affine.h), on the device against the CPU oracle
used as a general OSQP with l = u = -d_k on the dynamics rows (tests/affine_ref.py, pinned by tests/test_affine_ref.py): every kernel family
and every forced backend of tests/settings_cases.py at its smallest shape, a batch of three with a term per instance -- plain iterations, a
tight solve, export, zeros and clearing, no refactorization, the closed loop on the device in three forms, the adjoint, polish, the refusals
and the torch layer.  Run on the GPU box with:  python -m pytest tests -m gpu
"""
import ctypes as C
import warnings

import numpy as np
import pytest

import affine_ref as ar
import settings_cases as sc
from util import rel, forced, stacked_batch, rel1_any

pytestmark = pytest.mark.gpu

PAIRS = [(c, b) for c in ar.SCALE for b in sc.CASES[c]['backends']]
IDS = ['%s-%s' % (c, b or 'auto') for c, b in PAIRS]


def _batch(case, backend, factors=(1.0, 1.0, 1.0), setup=True, solve=False, **settings):
    """A BatchMPCController of three copies of the case (x0 scaled by ``factors``) on a forced backend, set up."""
    kw, attrs = sc.draw(case)
    nx = np.asarray(kw['Ad']).shape[0]
    kws = []
    for f in factors:
        d = dict(kw); d['x0'] = f * np.asarray(kw['x0'], dtype=float); d['Bd'] = np.asarray(kw['Bd'], dtype=float).reshape(nx, -1)
        for k in ('uref', 'uminus1', 'umin', 'umax', 'Dumin', 'Dumax'):
            if k in d:
                d[k] = np.atleast_1d(np.asarray(d[k], dtype=float))
        kws.append(d)
    with forced(backend, **{k: settings.pop(k) for k in ('tuning',) if k in settings}), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K = stacked_batch(kws, SOFT_ON=attrs.get('SOFT_ON', True), **settings)
        if setup:
            K.setup(solve=solve)
    return K


def _tight(case, backend, **more):
    return _batch(case, backend, eps_abs=ar.TIGHT, eps_rel=ar.TIGHT, max_iter=200000, **more)


def _rows(case):
    return (None, 1) if case in ar.ONE_ROW else (None,)


_iterates = {}


def _oracle_iterate(case, rows, b, iters=40):
    key = (case, rows, b)
    if key not in _iterates:
        Ko = ar.oracle(case, ar.term(case, rows)[b], eps=sc.EPS, solve=False)
        Ko.prob.iterate(iters)
        _iterates[key] = Ko.prob.iterate_state()[:3]
    return _iterates[key]


# ---- 1. plain iterations -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,backend', PAIRS, ids=IDS)
def test_plain_iterations_match_the_oracle(case, backend):
    """mpcqp_iterate(40) from the cold start with a term per instance: x, z, y as the oracle's, to the bound of the d-free problem
    (tests/test_gpu_backends.py: 1e-8 relative).  Without the feature the problem cannot be stated."""
    for rows in _rows(case):
        K = _batch(case, backend)
        K.set_affine(ar.term(case, rows))
        K.prob.iterate(40)
        x, z, y = K.prob.iterate_state()
        for b in range(ar.B):
            xo, zo, yo = _oracle_iterate(case, rows, b)
            ex, ez, ey = rel(x[b], xo), rel(z[b], zo), np.abs(y[b] - yo).max() / max(1.0, np.abs(yo).max())
            print('AFFINE_ITER %s/%s rows %s instance %d: x %.2e z %.2e y %.2e' % (case, backend or 'auto', rows or 'Np', b, ex, ez, ey))
            assert ex < 1e-8 and ez < 1e-8 and ey < 1e-8, (case, backend, rows, b, ex, ez, ey)


# ---- 2. tight solve and export --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,backend', PAIRS, ids=IDS)
def test_tight_solve_and_export(case, backend):
    """eps 1e-9: u0 within 1e-6 max(1e-3, |u0|) of the oracle's; mpcqp_export_qp shows 0.0 - d on the dynamics rows, bit for bit; the getter
    returns the term; every instance of the oracle is solved and has an active inequality row."""
    for rows in _rows(case):
        d = ar.term(case, rows)
        K = _tight(case, backend)
        K.set_affine(d)
        assert np.array_equal(K.affine(), d) and K.prob.affine_rows() == d.shape[1]
        K.solve()
        u0 = K.prob.u0()
        assert all(s == 'solved' for s in K.status()), K.status()
        _, _, _, l, u = K.prob.export_qp()
        ou = (K.Np + 1) * K.nx
        for b, (xo, yo, status, lo, uo) in enumerate(ar.tight(case, rows)):
            assert status == 'solved' and ar.active_inequalities(case, xo, lo, uo) >= 1, (case, rows, b, status)
            assert np.array_equal(l[b], np.clip(lo, -1e30, 1e30)) and np.array_equal(u[b], np.clip(uo, -1e30, 1e30)), (case, rows, b)
            err = np.abs(u0[b] - xo[ou:ou + K.nu]).max()
            print('AFFINE_TIGHT %s/%s rows %s instance %d: |u0 - oracle| %.2e' % (case, backend or 'auto', rows or 'Np', b, err))
            assert err <= 1e-6 * max(1e-3, np.abs(xo[ou:ou + K.nu]).max()), (case, backend, rows, b, err)


# ---- 3. zeros are nothing, and clearing works -----------------------------------------------------------------------------------------------
def _solve_and_loop(K):
    K.solve()
    x, y, info = K.prob.solution()
    out = dict(x=x, y=y, iter=np.array([i.iter for i in info]), status=np.array([i.status for i in info]))
    tr = K.run(sc.STEPS, w=np.repeat(sc.noise(K.nx)[:, None, :], ar.B, axis=1))
    out.update(x_traj=tr['x'], u_traj=tr['u'], st_traj=tr['status'], it_traj=tr['iter'])
    return out


@pytest.mark.parametrize('case,backend', PAIRS, ids=IDS)
def test_zeros_and_a_cleared_term_are_no_term(case, backend):
    """set_affine(zeros), and set_affine(None) after a nonzero term: the default-eps solve and a 6-step loop give the bits of a handle that
    never had a term."""
    base = _solve_and_loop(_batch(case, backend))
    for rows in _rows(case):
        Kz = _batch(case, backend)
        Kz.set_affine(np.zeros_like(ar.term(case, rows)))
        Kn = _batch(case, backend)
        Kn.set_affine(ar.term(case, rows))
        Kn.set_affine(None)
        assert Kn.affine() is None and Kz.prob.affine_rows() == (rows or Kz.Np)
        for K, what in ((Kz, 'zeros'), (Kn, 'cleared')):
            got = _solve_and_loop(K)
            for k in base:
                assert np.array_equal(base[k], got[k]), (case, backend, rows, what, k)


# ---- 4. no refactorization ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,backend', PAIRS, ids=IDS)
def test_a_term_costs_no_factorization(case, backend):
    """Without rho adaptation nothing but a changed row type refactors: across set_affine + solve the counter of mpcqp_get_stats does not move, and
    the handle's KKT solve (mpcqp_debug_kkt_solve: its factor) returns the bits it returned before -- the factor was not rewritten."""
    K = _batch(case, backend, adaptive_rho=0, max_iter=1000)
    rhs = np.random.default_rng(0).standard_normal((ar.B, K.prob.n))
    before, sol = K.prob.stats()[2], K.prob.kkt_solve(rhs)
    K.set_affine(ar.term(case))
    K.solve()
    K.prob.synchronize()
    st = K.prob.stats()
    assert st[2] == before and st[0] > 0, (case, backend, before, st)
    assert np.array_equal(sol, K.prob.kkt_solve(rhs)), (case, backend)


@pytest.mark.parametrize('case,backend', PAIRS, ids=IDS)
def test_zeros_move_no_counter_at_the_default_settings(case, backend):
    """Default settings (rho adaptation on): set_affine(zeros) + solve moves every counter of mpcqp_get_stats -- refactorizations among them -- exactly
    as the same solve without a term does."""
    K0, Kz = _batch(case, backend), _batch(case, backend)
    Kz.set_affine(np.zeros_like(ar.term(case)))
    for K in (K0, Kz):
        K.solve()
        K.prob.synchronize()
    assert K0.prob.stats() == Kz.prob.stats() and K0.prob.stats()[0] > 0, (case, backend)


def test_a_term_stays_across_update_model_and_update_settings():
    """Step data: after update_model (a new Ad) and update_settings the term is still the one that was set -- the getter, the exported l, u and the
    tight u0 against the oracle given the same model and term."""
    case = 'quadcopter'
    d = ar.term(case)
    Ad, Bd, _ = ar.plant(case)
    A2 = Ad * 0.98
    K = _tight(case, 'bcr8')
    K.set_affine(d)
    K.solve()
    K.update_model(Ad=np.stack([A2] * ar.B), solve=False)
    K.prob.update_settings(alpha=1.5)
    assert np.array_equal(K.affine(), d)
    K.solve()
    assert all(s == 'solved' for s in K.status())
    u0 = K.prob.u0()
    _, _, _, l, u = K.prob.export_qp()
    nx, Np = K.nx, K.Np
    for b in range(ar.B):
        Ko = sc.controller(case, 'default', True, eps=ar.TIGHT, max_iter=200000)
        Ko.Ad = A2
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            Ko.setup(solve=False)
            ar.put(Ko, d[b])
            Ko.solve()
        assert Ko.res.info.status == 'solved'
        assert np.array_equal(l[b][nx:(Np + 1) * nx], 0.0 - d[b].ravel()) and np.array_equal(u[b][nx:(Np + 1) * nx], 0.0 - d[b].ravel())
        assert np.abs(u0[b] - ar.u0_of(Ko)).max() <= 1e-6 * max(1e-3, np.abs(ar.u0_of(Ko)).max()), b


@pytest.mark.parametrize('case,backend', [('random_12_4_30_tight', 'bcr8'), ('random_12_4_30_tight', 'sweeps'), ('group_3_2_50_20_tight', None),
                                          ('wide_25_8_3_tight', None), ('point_mass', 'dense')])
def test_the_byte_and_work_models_count_the_term_only_where_there_is_one(case, backend):
    """mpcqp_get_stream_bytes / mpcqp_get_work: with a term per_solve grows by the 8 Np nx bytes read (per_iter by the same where the iterate is
    streamed from memory, nothing elsewhere); cleared, and with none ever set, they are what they were."""
    K = _batch(case, backend)
    nx, _, Np = ar.shape(case)
    base, work = K.prob.stream_bytes(), K.prob.mfma_per_iter()
    K.set_affine(ar.term(case))
    got = K.prob.stream_bytes()
    assert got[2] == base[2] + 8 * Np * nx and got[1] == base[1] and got[0] in (base[0], base[0] + 8 * Np * nx), (case, base, got)
    assert K.prob.mfma_per_iter() == work
    K.set_affine(ar.term(case, rows=1))
    assert K.prob.stream_bytes() == got                    # (one row is read Np times)
    K.set_affine(None)
    assert K.prob.stream_bytes() == base and K.prob.mfma_per_iter() == work


def test_instances_that_share_a_factor_take_different_terms():
    """mpcqp_share_factor: three instances of one model solve with ONE copy of its factor; with a term each, the results are those of the
    unshared run, bit for bit."""
    from pympc_amd import _lib
    case, d = 'random_12_4_30_tight', ar.term('random_12_4_30_tight')
    out = []
    for tuning in (0, _lib.TUNE_NO_SHARE):
        K = _batch(case, 'sweeps', tuning=tuning)
        if not tuning:
            assert K.share_factor() == ar.B
        K.set_affine(d)
        K.solve()
        x, y, info = K.prob.solution()
        out.append((x, y, bytes(info)))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
    assert not np.array_equal(out[0][0][0], out[0][0][1])          # (the instances do differ)


# ---- 5. the closed loop on the device --------------------------------------------------------------------------------------------------------
LOOPS = [('random_12_4_30_tight', 'bcr8'), ('random_12_4_30_tight', 'sweeps'), ('group_3_2_50_20_tight', None), ('wide_25_8_3_tight', None)]

@pytest.mark.parametrize('form', ar.FORMS)
@pytest.mark.parametrize('case,backend', LOOPS, ids=['%s-%s' % (c, b or 'auto') for c, b in LOOPS])
def test_device_loop_follows_the_oracle(case, backend, form):
    """Six steps of three instances under the disturbance of tests/settings_cases.py, eps 1e-9: a constant term; a schedule at hold = 1; a
    schedule at hold = 2 beside a model schedule.  x_traj and u_traj within 1e-6 relative of the oracle stepped in Python with the same
    indexing, every status 'solved'.  The handle is left with the last entry used."""
    d0, dt, hold, mt = ar.schedule(case, form)
    w = sc.noise(ar.shape(case)[0])
    K = _tight(case, backend, factors=ar.x0_factors(case))
    if d0 is not None:
        K.set_affine(d0)
    K.solve()
    tr = K.run(sc.STEPS, w=np.repeat(w[:, None, :], ar.B, axis=1), d_traj=dt, d_hold=hold, model_traj=mt)
    assert np.all(tr['status'] == 1), tr['status']
    last = d0 if dt is None else dt[(sc.STEPS - 1) // hold]
    assert np.array_equal(K.affine(), last)
    for b in range(ar.B):
        xo, uo, st = ar.oracle_loop(case, b, sc.STEPS, w, None if d0 is None else d0[b], None if dt is None else dt[:, b], hold,
                                    None if mt is None else (mt[0][:, b], mt[1][:, b]), 2)
        assert all(s == 'solved' for s in st), (case, form, b, st)
        ex, eu = rel1_any(tr['x'][:, b], xo), rel1_any(tr['u'][:, b], uo)
        print('AFFINE_LOOP %s/%s %s instance %d: x %.2e u %.2e' % (case, backend or 'auto', form, b, ex, eu))
        assert ex <= 1e-6 and eu <= 1e-6, (case, backend, form, b, ex, eu)


def test_a_constant_term_keeps_the_carry_and_a_schedule_switches_it_off():
    """bcr8: the constant-term loop with and without MPCQP_TUNE_NO_CARRY is bit-identical (what tests/test_gpu_loop_carry.py demands of a d-free
    loop); the carry counter moves without the flag, stays at zero with it and under a schedule of terms."""
    from pympc_amd import _lib
    case = 'random_12_4_30_tight'
    w = np.repeat(sc.noise(12)[:, None, :], ar.B, axis=1)
    runs, carried = [], []
    for tuning, sched in ((0, False), (_lib.TUNE_NO_CARRY, False), (0, True)):
        K = _batch(case, 'bcr8', factors=ar.x0_factors(case), tuning=tuning)
        assert '231' in K.prob.kernel_name(True).replace(' ', '')
        if not sched:
            K.set_affine(ar.term(case))
        K.solve()
        tr = K.run(sc.STEPS, w=w, d_traj=ar.term(case, entries=sc.STEPS) if sched else None)
        x, y, _ = K.prob.solution()
        runs.append(dict(tr, sol_x=x, sol_y=y))
        carried.append(K.prob.carry_stats()[0])
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k
    assert carried[0] > 0 and carried[1] == 0 and carried[2] == 0, carried


# ---- 6. the adjoint -------------------------------------------------------------------------------------------------------------------------
ADJOINT = [('random_5_3_8', 'bcr8'), ('random_12_4_30_tight', 'bcr8'), ('random_20_8_12_b', None)]


@pytest.mark.parametrize('case,backend', ADJOINT, ids=['%s-%s' % (c, b or 'auto') for c, b in ADJOINT])
def test_gradient_of_the_term(case, backend):
    """Tight solve; d_d is -d_l of tests/adjoint_ref.py on the affine l, u (1e-8, the level of tests/test_gpu_adjoint.py) on the rows behind
    stage 0 -- per row, and summed for a one-row term -- and the central differences of the oracle's tight u0 with respect to d to
    1e-4 max(1, |fd|), on the four largest entries of instance 0 and the largest of the one-row form (each form has one above 1e-3).  The step is 1e-3, a hundredth of the term's scale:
    the law is piecewise affine in d, so a central difference has no truncation error inside a region, and its noise is the tight solve's own
    error over the step -- 3e-9 on random_20_8_12_b (eps 1e-9 on residuals of a problem with a slack cost of 1e6), which a step of 1e-5 turns
    into 2.7e-4 of the difference (measured on the oracle alone: -1.2671342 at 1e-5, -1.2674025 at 1e-4, -1.2674115 at 1e-3)."""
    import adjoint_ref
    from adjoint_cases import device_state
    nx, nu, Np = ar.shape(case)
    g = np.random.default_rng(3).standard_normal((ar.B, nu))
    for rows in (None, 1):
        d = ar.term(case, rows)
        K = _tight(case, backend)
        K.set_affine(d)
        with pytest.raises(RuntimeError, match=r'\(-5\)'):            # MPCQP_ERR_STATE: the solution is not the new problem's
            K.prob.adjoint(g_u0=g, want=('x0',))
        K.solve()
        res = K.adjoint(g_u0=g, want=('d', 'x0', 'l', 'u'))
        assert np.all(res['status'] == 1), res['status']
        plain = K.adjoint(g_u0=g, want=('x0', 'l', 'u'))              # (mpcqp_adjoint itself, with the term in force)
        for k in ('x0', 'l', 'u'):
            assert np.array_equal(plain[k], res[k]), k
        for b in range(ar.B):
            st = list(device_state(K.prob, b))
            lo, uo = ar.tight(case, rows)[b][3:5]
            assert np.array_equal(st[2], np.clip(lo, -1e30, 1e30)) and np.array_equal(st[3], np.clip(uo, -1e30, 1e30))
            gw = np.zeros(K.prob.n); gw[(Np + 1) * nx:(Np + 1) * nx + nu] = g[b]
            ref = adjoint_ref.adjoint(*st, gw)
            want = -ref['d_l'][nx:(Np + 1) * nx].reshape(Np, nx)
            want = want if rows is None else want.sum(0, keepdims=True)
            err = rel1_any(res['d'][b], want.ravel())
            print('AFFINE_ADJ %s rows %s instance %d: %.2e (|d_d| %.2e)' % (case, rows or 'Np', b, err, np.abs(want).max()))
            assert err <= 1e-8, (case, rows, b, err)
        if True:                                                      # (both forms: the one-row term's largest entry too)
            dd = res['d'][0]
            top = np.argsort(-np.abs(dd))[:4 if rows is None else 1]
            assert np.abs(dd[top[0]]) > 1e-3, dd[top]
            h = 1e-3
            for e in top:
                u = []
                for s in (1.0, -1.0):
                    dp = d[0].copy().ravel(); dp[e] += s * h
                    u.append(ar.u0_of(ar.oracle(case, dp.reshape(-1, nx))))
                fd = g[0] @ (u[0] - u[1]) / (2 * h)
                print('AFFINE_FD %s entry %d: adjoint %.6e fd %.6e' % (case, e, dd[e], fd))
                assert abs(dd[e] - fd) <= 1e-4 * max(1.0, abs(fd)), (case, e, dd[e], fd)


# ---- 7. polish ------------------------------------------------------------------------------------------------------------------------------
def test_polish_reads_the_term():
    """random_12_4_30_tight with polish=True at eps 1e-3, as tests/test_gpu_polish.py holds its own cases.  At the x0 factors of
    affine_ref.POLISH_FACTORS -- where the CPU restatement accepts the polish from the ORACLE's iterate and lands on the optimum (asserted on the
    CPU) -- the device accepts it on all three instances and the polished u0 is within 1e-8 max(1, |u0|) of the optimum; the optimum is the
    oracle's eps 1e-9 solve polished on the CPU, the device solves at 1e-3.  At factor 1.0 the reference rejects it on all three: so does the
    device, and the result is the unpolished solve's, bit for bit.  On both batches the device's polish is the restatement on its own iterate and
    the affine l, u (status, x to 1e-9)."""
    import polish_ref
    case = 'random_12_4_30_tight'
    for factors, want in ((ar.POLISH_FACTORS, [1, 1, 1]), ((1.0, 1.0, 1.0), [-1, -1, -1])):
        ref = ar.polished(case, ar.TIGHT, factors)
        assert [s for _, s, _ in ar.polished(case, sc.EPS, factors)] == want
        K = _batch(case, 'bcr8', factors=factors, max_iter=200000)
        K.set_affine(ar.term(case))
        K.solve()
        assert all(s == 'solved' for s in K.status())
        raw = K.prob.solution()[0].copy()
        polish_ref.check_against_spec(K.prob)
        st, u0, x = K.prob.polish_status(), K.prob.u0(), K.prob.solution()[0]
        assert list(st) == want, (factors, st)
        Kp = _batch(case, 'bcr8', factors=factors, max_iter=200000, polish=True)      # ... and polish=True as a setting of the solve
        Kp.set_affine(ar.term(case))
        Kp.solve()
        assert list(Kp.prob.polish_status()) == want and np.array_equal(Kp.prob.solution()[0], x)
        for b, (uopt, _, _) in enumerate(ref):
            err = np.abs(u0[b] - uopt).max()
            print('AFFINE_POLISH factor %.1f instance %d: status %d, |u0 - opt| %.2e' % (factors[b], b, st[b], err))
            if want[b] == 1:
                assert err <= 1e-8 * max(1.0, np.abs(uopt).max()), (factors, b, err)
            else:
                assert np.array_equal(x[b], raw[b]), (factors, b)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_argument_and_state_errors():
    from pympc_amd import _lib
    from pympc_amd.solver import BatchProblem, DeviceProblem
    ARG, UNSUPPORTED, STATE = -1, -4, -5
    case = 'random_5_3_8'
    nx, nu, Np = ar.shape(case)
    L = _lib.load()
    bp = BatchProblem(ar.B, nx, nu, Np)
    d = ar.term(case)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rows = C.c_int()
    assert L.mpcqp_set_affine(bp._h, p(d), Np) == STATE and L.mpcqp_get_affine(bp._h, None, C.byref(rows)) == STATE      # before setup
    K = _tight(case, 'bcr8', solve=True)
    h = K.prob._h
    for bad in (2, Np + 1, -1):
        assert L.mpcqp_set_affine(h, p(d), bad) == ARG
    assert K.affine() is None
    io = _lib.AdjointIO(); io.struct_size = C.sizeof(_lib.AdjointIO)
    gu = np.ones((ar.B, nu)); io.g_u0 = p(gu)
    out = np.zeros((ar.B, Np * nx))
    assert L.mpcqp_adjoint_affine(h, C.byref(io), p(out)) == STATE and b'no affine term' in L.mpcqp_last_error()
    assert L.mpcqp_adjoint_affine(h, C.byref(io), None) == ARG
    # the schedule's refusals: before any launch, nothing changed
    lo = _lib.Loop()
    xt, ut = np.zeros((3, ar.B, nx)), np.zeros((2, ar.B, nu))
    stt, itt = np.zeros((2, ar.B), dtype=np.int32), np.zeros((2, ar.B), dtype=np.int32)
    lo.x_traj, lo.u_traj, lo.status_traj, lo.iter_traj = p(xt), p(ut), p(stt), p(itt)
    dt = ar.term(case, entries=2)

    def at(**over):
        a = _lib.AffineTraj()
        a.struct_size, a.hold, a.nentries, a.rows, a.d = C.sizeof(_lib.AffineTraj), 1, 2, Np, p(dt)
        for k, v in over.items():
            setattr(a, k, v)
        return a
    before = K.prob.solution()[0].copy()
    for a in (at(struct_size=16), at(hold=0), at(nentries=1), at(rows=2), at(d=None)):
        assert L.mpcqp_mpc_loop_affine(h, 2, C.byref(lo), None, C.byref(a)) == ARG, L.mpcqp_last_error()
    lo.ny = 1
    assert L.mpcqp_mpc_loop_affine(h, 2, C.byref(lo), None, C.byref(at())) == UNSUPPORTED
    lo.ny = 0
    assert K.affine() is None and np.array_equal(before, K.prob.solution()[0]) and not xt.any()
    assert L.mpcqp_mpc_loop_affine(h, 2, C.byref(lo), None, C.byref(at())) == 0 and xt.any()
    assert np.array_equal(K.affine(), dt[1])
    # the Python layer's own
    with pytest.raises(ValueError):
        K.set_affine(np.zeros((ar.B, 2, nx)))
    with pytest.raises(ValueError):
        K.run(2, d_traj=np.zeros((2, ar.B, 2, nx)))
    K.set_affine(None)
    with pytest.raises(RuntimeError, match='affine term'):
        K.adjoint(g_u0=gu, want=('d',))
    # raw-vector mode keeps refusing
    Kc = sc.controller(case, 'default', False)
    Kc.setup(solve=False)
    prob = DeviceProblem()
    prob.setup(Kc.P, Kc.q, Kc.A, Kc.l, Kc.u)
    with pytest.raises(RuntimeError, match=r'\(-5\)'):
        prob.set_affine(np.zeros(nx))


@pytest.mark.parametrize('form', ['rollout', 'rollout_tv', 'rollout_est', 'rollout_tv_est'])
def test_the_taped_rollouts_refuse_a_term(form):
    from pympc_amd.kalman import BatchLinearStateEstimator
    case = 'random_5_3_8'
    nx, nu, Np = ar.shape(case)
    K = _batch(case, 'bcr8', solve=True)
    Ad, Bd, x0 = ar.plant(case)
    sched = (np.stack([np.stack([Ad] * ar.B)] * 2), None, 1)
    Cm = np.stack([np.eye(2, nx)] * ar.B)
    est = lambda: BatchLinearStateEstimator(np.stack([x0] * ar.B), np.stack([Ad] * ar.B), np.stack([Bd] * ar.B), Cm, np.zeros((ar.B, nx, 2)))
    calls = dict(rollout=lambda: K.rollout(2), rollout_tv=lambda: K.rollout_tv(2, sched), rollout_est=lambda: K.rollout_est(2, est()),
                 rollout_tv_est=lambda: K.rollout_tv_est(2, sched, est()))
    if form in ('rollout', 'rollout_tv'):
        calls[form]()                                     # without a term: a tape, and its sweep works
        K.rollout_adjoint(g_u=np.ones((2, ar.B, nu)))
    K.set_affine(ar.term(case))
    K.solve()
    count = K.solve_count
    with pytest.raises(NotImplementedError, match='mpcqp_affine.h'):
        calls[form]()
    assert K.solve_count == count
    if form in ('rollout', 'rollout_tv'):                 # ... and the reverse sweep over the older tape refuses too (MPCQP_ERR_UNSUPPORTED)
        with pytest.raises(RuntimeError, match=r'\(-4\).*mpcqp_affine.h'):
            K.rollout_adjoint(g_u=np.ones((2, ar.B, nu)))


# ---- 9. the drop-in class and the torch layer -----------------------------------------------------------------------------------------------
def test_drop_in_controller_takes_the_term_with_update():
    """(On quadcopter, where the reference's two pins hold to 1e-6 -- tests/test_affine_ref.py; on random_5_3_8 two tight solves of one problem
    from two starts are 4e-5 apart in x_seq: its soft state box is violated by O(1).)"""
    case = 'quadcopter'
    nx, nu, Np = ar.shape(case)
    d = ar.term(case, rows=1)[0, 0]
    Ko = ar.oracle(case, d)
    with forced('bcr8'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K = sc.controller(case, 'default', False, eps=ar.TIGHT, max_iter=200000)
        K.setup()
        K.update(K.x0, d=d)
    assert K.res.info.status == 'solved'
    assert np.abs(K.output() - ar.u0_of(Ko)).max() <= 1e-6 * max(1e-3, np.abs(ar.u0_of(Ko)).max())
    assert np.array_equal(K.l, Ko.l) and np.array_equal(K.u, Ko.u)            # (the public l, u carry the term)
    _, info = K.output(return_x_seq=True)
    assert rel1_any(info['x_seq'], Ko.res.x[:(Np + 1) * nx].reshape(Np + 1, nx)) <= 1e-6
    ad = K.adjoint(g_u0=np.ones(nu), want=('d',))
    assert ad['d'].shape == (nx,) and ad['status'] == 1 and np.abs(ad['d']).max() > 0
    K.set_affine(None)
    K.update(K.x0)
    assert np.array_equal(K.l[nx:(Np + 1) * nx], np.zeros(Np * nx))


def test_torch_step_takes_the_term_and_differentiates_it():
    torch = pytest.importorskip('torch')
    from pympc_amd.torch_layer import mpc_step, mpc_rollout
    case = 'random_5_3_8'
    nx, nu, Np = ar.shape(case)
    d = ar.term(case)
    _, _, x0 = ar.plant(case)
    x = np.stack([x0] * ar.B)
    Ka, Kb = _tight(case, 'bcr8', solve=True), _tight(case, 'bcr8', solve=True)
    Ka.update(x, d=d, solve=False)
    ua = Ka.step(x)
    dev = torch.device('cuda')
    dt = torch.tensor(d, device=dev, requires_grad=True)
    xt = torch.tensor(x, device=dev)
    ub = mpc_step(Kb, xt, d=dt)
    assert np.array_equal(ub.detach().cpu().numpy(), ua)
    g = torch.tensor(np.random.default_rng(5).standard_normal((ar.B, nu)), device=dev)
    (gd,) = torch.autograd.grad((ub * g).sum(), dt)
    ref = Ka.adjoint(g_u0=g.cpu().numpy(), want=('d',))['d']
    assert gd.shape == dt.shape and np.array_equal(gd.cpu().numpy().reshape(ar.B, -1), ref) and np.abs(ref).max() > 0
    with pytest.raises(NotImplementedError, match='mpcqp_affine.h'):
        mpc_rollout(Kb, xt, 2)
