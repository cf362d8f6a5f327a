"""mpcqp_adjoint and mpcqp_gains on the shapes the golden fixtures do not reach (tests/adjoint_cases.py; pinned on the CPU by
tests/test_adjoint_cases.py): stages of 64 and 128, a last group of four columns that is partly empty, columns with slack variables and
with a held input at 32-wide stages, the fallback to one seed at a time where four columns do not fit a workgroup's LDS, a
grouped-eligible long shape with two inputs, an unsolved instance inside a column batch -- against the numpy restatement
(tests/adjoint_ref.py) on the device's own iterate and scaling, the column code against the single-vector code on the same factor, and
without side effects on the wide layouts.  One BatchMPCController per case, its seeds the instances: different models and active sets
in one launch.  Tolerance, settings and helpers are those of tests/test_gpu_adjoint.py (they live in tests/adjoint_cases.py)."""
import functools

import numpy as np
import pytest

import adjoint_cases as ac
import adjoint_ref as ar
from adjoint_cases import TOL, EPS, RAW, CHAINED, device_state, snapshot, same, case_batch
from util import rel1_any

pytestmark = pytest.mark.gpu
GAINS = (('x0', 'K_x0'), ('uminus1', 'K_um1'), ('xref', 'K_xref'), ('uref', 'K_uref'))


@functools.lru_cache(maxsize=None)
def _solved(name, backend=None):
    """The case's batch, solved, and what both calls return on it (computed once, read-only afterwards)."""
    K = case_batch(name, backend=backend)
    assert all(s == 'solved' for s in K.status()), (name, K.status())
    bp = K.prob
    g = np.random.default_rng(7).standard_normal((bp.batch, bp.n))
    got = bp.adjoint(g_w=g, want=CHAINED + RAW)
    info = bp.adjoint_info()
    Kgot = bp.gains()
    return K, g, got, info, Kgot, bp.adjoint_info()


@functools.lru_cache(maxsize=None)
def _maps(name, seed):
    return ar.parameter_maps(*ac.draw(name, seed))


@functools.lru_cache(maxsize=None)
def _oracle_masks(name, seed):
    """The active set the restatement finds on the CPU oracle's iterate at the same tolerance."""
    Ko = ac.oracle_controller(name, seed, EPS)
    assert Ko.res.info.status == 'solved'
    P, A, l, u, x, z, y, D, E, c = ac.oracle_state(Ko)
    return ar.active_rows(A, l, u, x, z, y, D, E, c)


# ---- 1. every output of both calls against the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(ac.CASES))
def test_adjoint_and_gains_are_the_restatement(name):
    K, g, got, (nact, nweak, status), Kgot, (nact2, nweak2, status2) = _solved(name)
    bp, case = K.prob, ac.CASES[name]
    errs = {}
    for b, seed in enumerate(case['seeds']):
        st = device_state(bp, b)
        maps = _maps(name, seed)
        ref = ar.adjoint(*st, g[b], maps)
        assert status[b] == 1 and nweak[b] == 0 and ref['n_weak'] == 0, (name, seed, status[b], nweak[b], ref['n_weak'])
        assert nact[b] == ref['n_active'], (name, seed, nact[b], ref['n_active'])
        olow, oupp = _oracle_masks(name, seed)
        assert np.array_equal(ref['low'], olow) and np.array_equal(ref['upp'], oupp), (name, seed)      # the device's iterate gives the oracle's set
        # ... and the kernel found it: a random seed leaves no active row's multiplier exactly zero, an inactive row's is exactly zero
        assert np.array_equal(got['l'][b] != 0.0, olow) and np.array_equal(got['u'][b] != 0.0, oupp), (name, seed)
        assert np.all(got['l'][b][~ref['low']] == 0.0) and np.all(got['u'][b][~ref['upp']] == 0.0), (name, seed)
        for k in CHAINED + RAW:
            errs[k] = max(errs.get(k, 0.0), rel1_any(got[k][b], ref['d_' + k if k in RAW else k]))
        Kref = ar.gains(*st, maps, (bp.Np + 1) * bp.nx, bp.nu)
        assert status2[b] == 1 and nweak2[b] == 0 and nact2[b] == Kref['n_active'], (name, seed)
        for k, kk in GAINS:
            errs[kk] = max(errs.get(kk, 0.0), rel1_any(Kgot[k][b], Kref[kk]))
    worst = max(errs.values())
    print('ADJOINT_ERR %s: max %.3e  %s' % (name, worst, ' '.join('%s=%.1e' % kv for kv in errs.items())))
    assert worst <= TOL, (name, errs)


# ---- 2. the column code against the single-vector code on the same factor -----------------------------------------------------------------
@pytest.mark.parametrize('name', [n for n, c in ac.CASES.items() if c['nu'] >= 2])
def test_gain_rows_are_the_adjoint_of_unit_seeds(name):
    K, _, _, _, Kgot, _ = _solved(name)
    bp = K.prob
    worst = 0.0
    for j in range(bp.nu):
        e = np.zeros((bp.batch, bp.nu)); e[:, j] = 1.0
        one = bp.adjoint(g_u0=e, want=CHAINED)
        assert np.all(bp.adjoint_info()[2] == 1), (name, j)
        for k in CHAINED:
            for b in range(bp.batch):
                worst = max(worst, rel1_any(Kgot[k][b, j], one[k][b]))
    print('ADJOINT_ROWS %s: largest difference between a gain row and adjoint(g_u0 = e_j) %.3e' % (name, worst))
    assert worst <= TOL, (name, worst)


# ---- 3. an unsolved neighbour inside a column batch -----------------------------------------------------------------------------------------
def test_unsolved_neighbour_in_a_column_batch():
    name, bad = ac.INFEASIBLE
    s = ac.CASES[name]['seeds']
    Ka, Kb = case_batch(name, (s[0], s[1], bad, s[2])), case_batch(name, (s[0], s[1], s[2]))
    assert Ka.status() == ['solved', 'solved', 'primal infeasible', 'solved'], Ka.status()
    assert Kb.status() == ['solved'] * 3
    ga = np.random.default_rng(7).standard_normal((4, Ka.prob.n))
    ra, rb = Ka.prob.adjoint(g_w=ga, want=CHAINED + RAW), Kb.prob.adjoint(g_w=ga[[0, 1, 3]], want=CHAINED + RAW)
    sa, sb = Ka.prob.adjoint_info()[2], Kb.prob.adjoint_info()[2]
    assert list(sa) == [1, 1, 0, 1] and list(sb) == [1, 1, 1], (sa, sb)
    Ga, Gb = Ka.gains(), Kb.gains()
    assert list(Ga['status']) == [1, 1, 0, 1] and list(Gb['status']) == [1, 1, 1]
    for k in CHAINED + RAW:
        assert np.all(ra[k][2] == 0.0), k
        assert np.array_equal(ra[k][[0, 1, 3]], rb[k]), k
        assert np.all(np.isfinite(ra[k])), k
    assert all(np.any(rb[k][b] != 0.0) for k in ('x0', 'q', 'l') for b in range(3))
    for k in ('K_x0', 'K_um1', 'K_xref', 'K_uref'):
        assert np.all(Ga[k][2] == 0.0), k
        assert np.array_equal(Ga[k][[0, 1, 3]], Gb[k]), k
    assert np.any(Gb['K_x0'] != 0.0)


# ---- 4. no side effects on the wide layouts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['nb64_nu6', 'nb128_nu5'])
def test_wide_layouts_are_left_as_they_were(name):
    Ka, Kb = case_batch(name), case_batch(name)
    bp = Ka.prob
    rhs = np.random.default_rng(0).standard_normal((bp.batch, bp.n))
    before, snap = bp.kkt_solve(rhs), snapshot(bp)
    assert same(snap, snapshot(Kb.prob))
    g = np.random.default_rng(3).standard_normal((bp.batch, bp.n))
    bp.adjoint(g_w=g, g_u0=np.ones((bp.batch, bp.nu)), want=CHAINED + RAW)
    assert np.all(Ka.gains()['status'] == 1)
    assert np.array_equal(before, bp.kkt_solve(rhs))                  # the handle's own factor is untouched
    assert same(snap, snapshot(bp))
    # the next update and solve, against the twin that never took an adjoint
    x1 = np.asarray(Ka.x0) * 0.9
    for K in (Ka, Kb):
        K.update(x1)
    assert same(snapshot(Ka.prob), snapshot(Kb.prob))
    assert np.array_equal(Ka.prob.kkt_solve(rhs), Kb.prob.kkt_solve(rhs))


# ---- 5. the sweeps backend forced ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['long100_nu2', 'nb16_nu5'])
def test_forced_sweeps_backend_gives_the_same(name):
    """The adjoint's own factor is generic: a backend differs only through the iterate that fixes the active set."""
    _, g, got, info, Kgot, _ = _solved(name)
    Ks, gs, gots, infos, Kgots, _ = _solved(name, 'sweeps')
    assert np.array_equal(g, gs) and np.array_equal(info[0], infos[0])
    assert np.all(infos[2] == 1) and np.all(infos[1] == 0)
    for k in ('l', 'u'):
        assert np.array_equal(got[k] != 0.0, gots[k] != 0.0), k      # the same active masks
    worst = max([rel1_any(gots[k], got[k]) for k in CHAINED + RAW] + [rel1_any(Kgots[k], Kgot[k]) for k in CHAINED])
    print('ADJOINT_SWEEPS %s: largest difference to the automatic backend %.3e' % (name, worst))
    assert worst <= TOL, (name, worst)
