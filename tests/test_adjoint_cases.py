"""The case table of tests/adjoint_cases.py, pinned on the CPU before any GPU is involved: every (case, seed) is a usable input for a value
comparison -- solved, inequalities active, no weakly active row, well-conditioned active rows, the same active set at a tighter tolerance --
and the restatement tests/adjoint_ref.py is right on these shapes too (central finite differences of the CPU oracle, as
tests/test_adjoint_reference.py does on the golden shapes).  tests/test_gpu_adjoint_shapes.py holds the device to the restatement on them."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import adjoint_cases as ac
import adjoint_ref as ar
import adjoint_sweeps

IDS = ['%s-%d' % p for p in ac.pairs()]


@functools.lru_cache(maxsize=None)
def _solved(name, seed, eps):
    K = ac.oracle_controller(name, seed, eps)
    assert K.res.info.status == 'solved', (name, seed, K.res.info.status)
    return K


def test_the_table_is_complete():
    """Two to four seeds per case; the widths, the groups of four and the LDS arithmetic the table's comments claim."""
    assert len(ac.CASES) == 13
    for name, c in ac.CASES.items():
        assert 2 <= len(c['seeds']) <= 4 and len(set(c['seeds'])) == len(c['seeds']), name
        assert c['Nc'] <= c['Np']
    nb = {n: ac.stage_width(n) for n in ac.CASES}
    assert {n for n, v in nb.items() if v > 32} == set(ac.WIDE) and nb['nb128_nu5'] == 128 and nb['nb64_nu6'] == nb['nb64_nu10_held'] == 64
    assert all(nb[n] == 32 for n in ('nb32_nu5_soft', 'nb32_nu9_held', 'nb32_nu2', 'nb32_np60'))
    assert {ac.CASES[n]['nu'] % 4 for n in ac.CASES if nb[n] <= 16} >= {1, 2, 3}             # every partly filled last group of columns
    for n in ac.FALLBACK:                                                                    # above one workgroup's LDS on the columns alone
        assert ac.CASES[n]['nu'] > 1 and nb[n] <= 32 and ac.column_bytes(n) > 160 * 1024, (n, ac.column_bytes(n))
        assert len(ac.CASES[n]['seeds']) == 2                                                # (the long ones: two instances)
    for n in set(ac.CASES) - set(ac.FALLBACK) - set(ac.WIDE):
        assert ac.column_bytes(n) < 160 * 1024, (n, ac.column_bytes(n))
    # the row count column_bytes() works with is the builder's
    for n in ('long_nu3_held', 'nb16_nu7_hard'):
        K = ac.oracle_controller(n, ac.CASES[n]['seeds'][0], 1e-3)
        assert 32 * (K.A.shape[0] + (K.Np + 1) * nb[n] + 2) == ac.column_bytes(n), n


@pytest.mark.parametrize('name,seed', ac.pairs(), ids=IDS)
def test_every_case_and_seed_is_usable(name, seed):
    K = _solved(name, seed, 1e-9)
    P, A, l, u, x, z, y, D, E, c = st = ac.oracle_state(K)
    low, upp = ar.active_rows(A, l, u, x, z, y, D, E, c)
    eq = np.clip(l, -1e30, 1e30) == np.clip(u, -1e30, 1e30)
    nineq = int(np.count_nonzero((low | upp) & ~eq))
    assert nineq >= 2, (name, seed, nineq)
    # 1000 x the device's weak_tol: a device iterate that differs at 1e-9 cannot cross it
    assert ar.count_weak(l, u, z, y, weak_tol=1e-3) == 0, (name, seed)
    sv = np.linalg.svd(A.toarray()[low | upp], compute_uv=False)
    print('%s seed %d: %d active inequalities, sigma_min / sigma_max = %.2e' % (name, seed, nineq, sv[-1] / sv[0]))
    assert sv[-1] / sv[0] >= 1e-4, (name, seed, sv[-1] / sv[0])
    K11 = _solved(name, seed, 1e-11)
    el, eu = ar.exact_active_rows(A, l, u, K11.res.x, K11.res.y)
    assert np.array_equal(low, el) and np.array_equal(upp, eu), (name, seed)


def test_the_unsolved_neighbour_is_primal_infeasible():
    K = ac.oracle_controller(*ac.INFEASIBLE, 1e-9)
    assert K.res.info.status == 'primal infeasible', K.res.info.status


def _fd(name, seed, param, h=1e-5, eps=1e-11):
    """du_0 / d(param) by central differences of cold oracle solves at eps (tests/test_adjoint_reference.py: both ends of a difference
    follow the same iteration path, so their solver errors largely cancel)."""
    from pympc_amd import MPCController
    from oracle.osqp_oracle import OSQP
    import warnings
    kw, attrs = ac.draw(name, seed)
    nu = kw['Bd'].shape[1]
    base = np.asarray(kw[param], dtype=float)
    J = np.zeros((nu, base.size))

    def u0(v):
        K = MPCController(eps_abs=eps, eps_rel=eps, **dict(kw, **{param: v}))
        for a, val in attrs.items():
            setattr(K, a, val)
        K.prob = OSQP(); K.solver_settings = dict(max_iter=4000000)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            K.setup()
        assert K.res.info.status == 'solved'
        ou = (K.Np + 1) * K.nx
        return K.res.x[ou:ou + nu].copy()

    pts = []
    for j in range(base.size):
        e = np.zeros(base.size); e[j] = h
        pts += [base + e, base - e]
    with ThreadPoolExecutor(max_workers=8) as pool:        # (independent solves, each in its own oracle workspace; the C call releases the GIL)
        us = list(pool.map(u0, pts))
    for j in range(base.size):
        J[:, j] = (us[2 * j] - us[2 * j + 1]) / (2 * h)
    return J


@pytest.mark.parametrize('name,params', [('nb16_nu6', ('x0',)), ('nb32_nu9_held', ('x0', 'uminus1')), ('nb64_nu10_held', ('x0',)),
                                         ('nb128_nu5', ('x0',))])
def test_restatement_against_finite_differences_on_these_shapes(name, params):
    """K_x0 (and K_um1 where a held input changes the Delta-u rows) against central differences of the oracle: h = 1e-5, eps 1e-11, cold
    solves, tolerance 1e-4 max(1, |J|_inf) -- method and bound of test_restatement_against_finite_differences."""
    seed = ac.CASES[name]['seeds'][0]
    K = _solved(name, seed, 1e-11)
    kw, attrs = ac.draw(name, seed)
    G = ar.gains(*ac.oracle_state(K), ar.parameter_maps(kw, attrs), (K.Np + 1) * K.nx, K.nu)
    assert G['n_weak'] == 0
    for param in params:
        J = _fd(name, seed, param)
        got = G[{'x0': 'K_x0', 'uminus1': 'K_um1'}[param]]
        err = np.abs(got - J).max()
        print('%s seed %d: |K_%s - FD|_inf = %.3e, |J|_inf = %.3e' % (name, seed, param, err, np.abs(J).max()))
        assert err <= 1e-4 * max(1.0, np.abs(J).max()), (name, param, err)


@pytest.mark.parametrize('name', ['nb32_nu2', 'nb64_nu6', 'nb128_nu5'])
def test_the_sweeps_as_designed_reach_the_tolerance_on_slack_held_rows(name):
    """In these cases states start outside their soft box: active state-box rows that only their slack variable can satisfy, whose
    multipliers the regularized sweeps contract by about 0.5 a sweep (eps_feas against delta).  The sweeps of DESIGN.md section 5f with exact
    inner solves (tests/adjoint_sweeps.py) must reach the device tests' tolerance, 1e-9 of max(1, |.|_inf), within refine_iter + extra_iter
    sweeps for every unit seed of u_0: the stopping rule and its budget are right for such rows (a rule that stopped where a correction
    failed to halve left K_um1 4.6e-2 off here)."""
    for seed in ac.CASES[name]['seeds']:
        K = _solved(name, seed, 1e-9)
        P, A, l, u, x, z, y, D, E, c = ac.oracle_state(K)
        low, upp = ar.active_rows(A, l, u, x, z, y, D, E, c)
        slack = K.res.x[(K.Np + 1) * K.nx + K.Nc * K.nu:]
        assert np.abs(slack).max() > 0.1, (name, seed)                     # a violated soft box: the case is what it is there for
        ou, worst, most = (K.Np + 1) * K.nx, 0.0, 0
        for j in range(K.nu):
            g = np.zeros(P.shape[0]); g[ou + j] = 1.0
            rw, ry = ar.solve_adjoint(P, A, low, upp, g, D, E, c)
            xs, ys, k = adjoint_sweeps.sweeps(P, A, low, upp, g, D, E, c)
            worst = max(worst, np.abs(xs - rw).max() / max(1.0, np.abs(rw).max()), np.abs(ys - ry).max() / max(1.0, np.abs(ry).max()))
            most = max(most, k)
        print('%s seed %d: emulated sweeps at most %d, largest error %.2e' % (name, seed, most, worst))
        assert worst <= 1e-9 and most <= 64, (name, seed, worst, most)
