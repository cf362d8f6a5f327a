"""The device solver under non-default OSQP settings, against the CPU oracle (oracle/osqp_ref.c) on the table of tests/settings_cases.py -- which
tests/test_settings_cases.py pins on the oracle first: every listed (case, setting) keeps its (status, iter, rho_updates) across eps (1 +- 0.03),
so a rounding-level difference on the device cannot move a count.  Every field of mpcqp_settings that reaches a kernel is exercised on every
kernel family with an ADMM body or a check of its own: round lengths of 1, 7 and 10 iterations, stops that are a rho estimate only, no
relaxation and more of it, other sigma / rho / scaling, no adaptation, many refactorizations, no termination test until the end, iteration
limits off the round -- cold solves, plain iterates, the closed loop on the device with and without its carry, warm_start = 0, the
infeasibility tolerance, and settings changed between two solves of one handle.  The tolerances are the suite's own for the same comparisons
at the defaults (tests/test_gpu_gaps.py, tests/test_gpu_parity.py, tests/test_gpu_backends.py).
Run on the GPU box with:  python -m pytest tests -m gpu
"""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import settings_cases as sc
from util import rel, forced, stacked_batch, bcr_schedule, shape_of

pytestmark = pytest.mark.gpu


def _bcr_schedule(case):
    return bcr_schedule(*shape_of(sc.draw(case)[0]))


def assert_backend(case, backend, bp):
    """kernel_name() shows the forced backend; for a backend mpcqp_create picked, the kernel family the case is in the table for."""
    kn = bp.kernel_name(loop=False)
    mode = kn.split(',')[4]
    if backend is not None:
        held = sc.draw(case)[0].get('Nc') not in (None, sc.draw(case)[0]['Np'])      # (a held input: the sweeps with their bordered correction)
        want = {'sweeps': '1' if held else '0', 'dense': '2', 'bcr': str(100 + _bcr_schedule(case)), 'bcr8': str(200 + _bcr_schedule(case)), 'bcrt': str(200 + _bcr_schedule(case))}[backend]
        assert mode == want and kn.startswith('w8::') == (backend == 'bcr8'), (case, backend, kn)
        return
    fam = sc.CASES[case]['family']
    if fam == 'grouped':
        kw, _ = sc.draw(case)
        nx, nu = np.asarray(kw['Bd']).shape
        g = 16 // (nx + nu)
        assert bp.factor_doubles == (-(-(kw['Np'] + 1) // g) + 1) * 768, (case, bp.factor_doubles)      # (tests/test_gpu_group.py: _grouped)
    else:
        assert kn.startswith('k_mpc_run<%d,' % {'nb32': 32, 'wide64': 64, 'wide128': 128}[fam]), (case, kn)


def _device(case, backend, setting, solve=True, **more):
    with forced(backend), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K = sc.controller(case, setting, False, **more)
        K.setup(solve=solve)
    return K


# ---- 1. cold solves ---------------------------------------------------------------------------------------------------------------------
COLD = sc.device_pairs()


@pytest.mark.parametrize('case,backend,setting', COLD, ids=['%s-%s-%s' % (c, b or 'auto', s) for c, b, s in COLD])
def test_cold_solve_has_the_oracles_counts_and_iterate(case, backend, setting):
    """status, iter and rho_updates equal the oracle's; x within 1e-6 max(1, |x_oracle|_inf) (tests/test_gpu_gaps.py:122).
    (What the chk0 / max40 / max60 cases caught: a check body that went straight to the 10x test at an unchecked iteration limit reported
    'solved inaccurate' where OSQP says 'solved' -- 41 of these cases.  Under chk0 the oracle also makes a rho update ON the limit, iteration
    400, on random_5_3_8, random_12_4_30_hard and two of the *_tight instances: a check body that ends the run before that estimate cannot
    have their rho_updates.)"""
    want, xo = sc.oracle_solve(case, setting)
    K = _device(case, backend, setting)
    assert_backend(case, backend, K.prob.batch_problem)
    got = sc.triple(K.res.info)
    err = np.abs(K.res.x - xo).max() / max(1.0, np.abs(xo).max())
    print('SETTINGS_COLD %s/%s/%s: device %s oracle %s x err %.2e' % (case, backend or 'auto', setting, got, want, err))
    assert got == want, (case, backend, setting, got, want)
    assert err <= 1e-6, (case, backend, setting, err)


# ---- 2. plain iterates, scaling and the KKT solve under the settings that change the iteration or the factor ---------------------------------
PLAIN_CASES = {}
for _c, _d in sc.CASES.items():
    PLAIN_CASES.setdefault(_d['family'], _c)               # (the family's first case, on every backend it has in the table)
PLAIN = [(c, b, s) for c in PLAIN_CASES.values() for b in sc.CASES[c]['backends'] for s in sc.ITERATION_SETTINGS]


@pytest.mark.parametrize('case,backend,setting', PLAIN, ids=['%s-%s-%s' % (c, b or 'auto', s) for c, b, s in PLAIN])
def test_scaling_iterates_and_kkt_solve_match_the_oracle(case, backend, setting):
    """D, E, c to 1e-12 (tests/test_gpu_parity.py:80), exactly 1 without equilibration; iterate(n), n = 1, 7, 40, to 1e-8 and the reduced KKT solve
    against dense numpy to 1e-8 (tests/test_gpu_backends.py:85-116), with the setting's sigma and rho in the matrix."""
    st = sc.settings(setting)
    K = _device(case, backend, setting, solve=False)
    bp = K.prob.batch_problem
    D, E, c, rho = bp.scaling()
    Do, Eo, co = sc.oracle_iterate(case, setting, 1)[3]
    assert rel(D[0], Do) < 1e-12 and rel(E[0], Eo) < 1e-12 and abs(c[0] - co) / co < 1e-12
    if setting == 'scaling0':
        assert (D[0] == 1.0).all() and (E[0] == 1.0).all() and c[0] == 1.0
    assert rho[0] == st.get('rho', 0.1)
    # the reduced KKT matrix c P + sigma D^-2 + A' diag(rho E^2) A on the host-built matrices
    sigma = st.get('sigma', 1e-6)
    U = sp.triu(K.P).toarray(); P = U + np.triu(U, 1).T
    A = K.A.toarray()
    l, u = np.clip(K.l, -1e30, 1e30), np.clip(K.u, -1e30, 1e30)
    ls, us = E[0] * l, E[0] * u
    rho_vec = np.where((ls < -1e26) & (us > 1e26), 1e-6, np.where(us - ls < 1e-4, 1e3 * rho[0], rho[0]))
    Kmat = c[0] * P + np.diag(sigma / D[0] ** 2) + A.T @ np.diag(rho_vec * E[0] ** 2) @ A
    rng = np.random.default_rng(5)
    for _ in range(2):
        rhs = rng.standard_normal(P.shape[0])
        sol = bp.kkt_solve(rhs[None])[0]
        assert rel(sol, np.linalg.solve(Kmat, rhs)) < 1e-8, (case, backend, setting)
    for n in (1, 7, 40):
        Kn = _device(case, backend, setting, solve=False)
        Kn.prob.batch_problem.iterate(n)
        x, z, y = Kn.prob.batch_problem.iterate_state()
        xo, zo, yo, _ = sc.oracle_iterate(case, setting, n)
        assert rel(x[0], xo) < 1e-8 and rel(z[0], zo) < 1e-8, (case, backend, setting, n, rel(x[0], xo), rel(z[0], zo))
        assert np.abs(y[0] - yo).max() < 1e-8 * max(1.0, np.abs(yo).max()), (case, backend, setting, n)


# ---- 3. the closed loop on the device -----------------------------------------------------------------------------------------------------
def _batch(case, setting, **more):
    kw, attrs = sc.draw(case)
    kws = []
    for f in sc.LOOPS[(case, setting)]:
        d = dict(kw); d['x0'] = f * np.asarray(kw['x0'], dtype=float); d['Bd'] = np.asarray(kw['Bd'], dtype=float).reshape(len(d['x0']), -1)
        for k in ('uref', 'uminus1', 'umin', 'umax', 'Dumin', 'Dumax'):
            d[k] = np.atleast_1d(np.asarray(d[k], dtype=float))
        kws.append(d)
    return stacked_batch(kws, SOFT_ON=attrs.get('SOFT_ON', True), **dict(sc.settings(setting), **more)), kws


LOOPS = sc.device_loops()


@pytest.mark.parametrize('case,backend,setting', LOOPS, ids=['%s-%s-%s' % (c, b or 'auto', s) for c, b, s in LOOPS])
def test_device_loop_follows_the_oracle_step_by_step(case, backend, setting):
    """BatchMPCController.run(6, w) on three copies with different x0; the oracle steps alongside on the device's own trajectory
    (tests/test_gpu_gaps.py:203-213): every step's (iter, status) is equal, u within 1e-7 max(1e-3, |u|); the same run with
    MPCQP_TUNE_NO_CARRY is bit-identical."""
    from pympc_amd import _lib
    runs = []
    for tuning in (0, _lib.TUNE_NO_CARRY):
        with forced(backend, tuning=tuning), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            K, kws = _batch(case, setting)
            K.setup()
            assert_backend(case, backend, K.prob)
            first = [(i.iter, i.status) for i in K.prob.infos()]
            nx = kws[0]['Ad'].shape[0]
            w = np.ascontiguousarray(np.broadcast_to(sc.noise(nx)[:, None, :], (sc.STEPS, len(kws), nx)))
            tr = K.run(sc.STEPS, w=w)
        runs.append((first, tr))
    (first, tr), (first_nc, tr_nc) = runs
    assert first == first_nc and sorted(tr) == sorted(tr_nc)
    for k in tr:
        assert np.array_equal(tr[k], tr_nc[k], equal_nan=True), (case, backend, setting, k)
    for i, f in enumerate(sc.LOOPS[(case, setting)]):
        Ko = sc.controller(case, setting, True, x0=kws[i]['x0'].copy())
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            Ko.setup()
            assert (Ko.res.info.iter, Ko.res.info.status_val) == first[i], (case, backend, setting, i, 'setup')
            for k in range(sc.STEPS):
                uo = np.atleast_1d(Ko.output())
                assert np.abs(tr['u'][k, i] - uo).max() <= 1e-7 * max(1e-3, np.abs(uo).max()), (case, backend, setting, i, k)
                Ko.update(tr['x'][k + 1, i], tr['u'][k, i])
                assert (Ko.res.info.iter, Ko.res.info.status_val) == (tr['iter'][k, i], tr['status'][k, i]), (case, backend, setting, i, k)


# ---- 4. warm_start = 0 through the seam a caller can set it on ----------------------------------------------------------------------------
@pytest.mark.parametrize('case,backend', [('cart_pole', 'dense'), ('random_12_4_30', 'bcr8')])
def test_warm_start_off_starts_every_solve_from_zero(case, backend):
    """DeviceProblem().setup(P, q, A, l, u, warm_start=False) against OSQP().setup(..., warm_start=False): solve, update(q, l, u) to the next
    state, solve.  Both solves have the oracle's counts and its x to 1e-6 max(1, |x|_inf).  The counts alone cannot tell a cold second solve from
    a warm one on these two cases (25 / 25 and 50 / 50 iterations on the oracle), the iterate it ends on can: the oracle's two second solutions
    differ by 1.6e-2 and 4.3e-5 relative, which the test checks first."""
    from pympc_amd.solver import DeviceProblem
    from oracle.osqp_oracle import OSQP
    kw, _ = sc.draw(case)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        Kh = sc.controller(case, 'default', True); Kh.setup()      # (the host build of P, q, A, l, u, and the next state)
        P, A, q0, l0, u0 = Kh.P, Kh.A, Kh.q.copy(), Kh.l.copy(), Kh.u.copy()
        u = np.atleast_1d(Kh.output())
        x1 = np.asarray(kw['Ad']) @ kw['x0'] + np.asarray(kw['Bd'], dtype=float).reshape(len(kw['x0']), -1) @ u
        Kh.update(x1, u)
        q1, l1, u1 = Kh.q.copy(), Kh.l.copy(), Kh.u.copy()
        ref = {}
        for ws in (False, True):
            O = OSQP(); O.setup(P, q0, A, l0, u0, warm_start=ws, eps_abs=sc.EPS, eps_rel=sc.EPS)
            a = O.solve(); O.update(q=q1, l=l1, u=u1); b = O.solve()
            ref[ws] = (a, b)
        assert rel(ref[True][1].x, ref[False][1].x) > 1e-5                  # (a warm second solve would be seen)
        with forced(backend):
            dev = DeviceProblem()
            dev.setup(P, q0, A, l0, u0, warm_start=False, eps_abs=sc.EPS, eps_rel=sc.EPS)
            assert_backend(case, backend, dev.batch_problem)
            ra = dev.solve(); dev.update(q=q1, l=l1, u=u1); rb = dev.solve()
    for got, want in ((ra, ref[False][0]), (rb, ref[False][1])):
        assert sc.triple(got.info) == sc.triple(want.info), (case, sc.triple(got.info), sc.triple(want.info))
        assert np.abs(got.x - want.x).max() <= 1e-6 * max(1.0, np.abs(want.x).max()), case


# ---- 5. the infeasibility tolerance -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('st', [dict(eps_prim_inf=1e-7), dict(check_termination=7), dict(eps_prim_inf=1e-7, check_termination=7)],
                         ids=['eps_prim_inf1e-7', 'chk7', 'eps_prim_inf1e-7_chk7'])


def test_primal_infeasibility_is_reported_where_the_oracle_reports_it(st):
    """The infeasible point mass of tests/test_gpu_parity.py:172-187: 'primal infeasible' at 75 iterations with eps_prim_inf = 1e-7 (25 at the
    default), at 28 with check_termination = 7, at 119 after four rho updates with both (tests/test_settings_cases.py pins the oracle's
    numbers); x is NaN and output() is uref."""
    from pympc_amd import fixtures
    K, Ko = sc.infeasible_point_mass(False, **st), sc.infeasible_point_mass(True, **st)
    assert Ko.res.info.status == 'primal infeasible'
    assert sc.triple(K.res.info) == sc.triple(Ko.res.info), (sc.triple(K.res.info), sc.triple(Ko.res.info))
    assert np.all(np.isnan(K.res.x))
    assert np.array_equal(K.output(), fixtures.point_mass()['uref'])


# ---- 6. update_settings between two solves of one handle ----------------------------------------------------------------------------------
NEW = dict(check_termination=7, alpha=1.8, max_iter=500, eps_prim_inf=1e-3)


@pytest.mark.parametrize('case,backend', [('cart_pole', 'dense'), ('random_12_4_30', 'bcr8'), ('random_20_8_12', None)])
def test_settings_changed_between_solves_take_effect(case, backend):
    """setup and solve with adaptive_rho = 0; update_settings(check_termination=7, alpha=1.8, max_iter=500, eps_prim_inf=1e-3); warm_start(x, y) with
    the first solution; update() to the next state and solve -- against the oracle set up with those settings from the start and warm-started with
    the same (x, y): status and iter equal, x within 1e-6 max(1, |x|_inf).  (The oracle here: 42 and 70 iterations, and on random_20_8_12 the new
    limit of 500 -- the default round would give 50 / 75 / 4000.)"""
    kw, _ = sc.draw(case)
    K = _device(case, backend, 'default', adaptive_rho=0)
    assert_backend(case, backend, K.prob.batch_problem)
    x1, y1 = np.array(K.res.x), np.array(K.res.y)
    u = np.atleast_1d(K.output())
    xn = np.asarray(kw['Ad']) @ kw['x0'] + np.asarray(kw['Bd'], dtype=float).reshape(len(kw['x0']), -1) @ u
    K.prob.update_settings(adaptive_rho_interval=28, **NEW)        # (the interval given explicitly: what 0 resolves to after such a change is not defined)
    Ko = sc.controller(case, 'default', True, adaptive_rho=0, adaptive_rho_interval=28, **NEW)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K.prob.warm_start(x1, y1)
        K.update(xn, u)
        Ko.setup(solve=False)
        Ko.prob.warm_start(x1, y1)
        Ko.update(xn, u)
    got, want = sc.triple(K.res.info), sc.triple(Ko.res.info)
    print('SETTINGS_UPDATE %s: device %s oracle %s' % (case, got, want))
    assert got[:2] == want[:2], (case, got, want)
    assert want[1] % 7 == 0 or want[1] == 500, want
    assert np.abs(K.res.x - Ko.res.x).max() <= 1e-6 * max(1.0, np.abs(Ko.res.x).max()), case
