"""The table of tests/settings_cases.py pinned on the CPU oracle: every listed pair and loop keeps its counts across the tolerance band, every
setting is listed for every kernel family and can be told from the defaults where it is listed, the paths the settings are named for are taken,
and a run whose last iteration was not a checked one ends as osqp_solve ends it (oracle/osqp_ref.c).  No GPU needed."""
import pytest

import settings_cases as sc
from util import rel


@pytest.mark.parametrize('case,setting', sc.pairs(), ids=['%s-%s' % p for p in sc.pairs()])
def test_every_listed_pair_keeps_its_counts_across_the_band(case, setting):
    ok, t = sc.stable(case, setting)
    print('SETTINGS_CASE %s/%s: %s' % (case, setting, t))
    assert ok, (case, setting, t)


@pytest.mark.parametrize('case,setting', [(c, s) for s, cs in sc.MOVES.items() for c in cs])
def test_every_pair_left_out_for_moving_does_move(case, setting):
    """(so that the list of exclusions cannot outlive its reason)"""
    ok, t = sc.stable(case, setting)
    assert not ok, (case, setting, t)


@pytest.mark.parametrize('case,setting', [(c, s) for s, cs in sc.SAME_AS_DEFAULT.items() for c in cs])
def test_every_pair_left_out_as_the_defaults_is_the_defaults(case, setting):
    assert sc.stable(case, setting)[0] and not _told_from_the_defaults(case, setting)[0], (case, setting)


@pytest.mark.parametrize('case,setting', list(sc.LOOPS), ids=['%s-%s' % p for p in sc.LOOPS])
def test_every_listed_loop_keeps_its_counts_across_the_band(case, setting):
    ok, t = sc.loop_stable(case, setting)
    print('SETTINGS_LOOP %s/%s: %s' % (case, setting, t[0]))
    assert ok, (case, setting, t)
    assert len(set(sc.LOOPS[(case, setting)])) == 3


def test_every_setting_is_listed_for_every_family():
    assert {c['family'] for c in sc.CASES.values()} == set(sc.FAMILIES)
    for s in sc.SETTINGS:
        got = {sc.CASES[c]['family'] for c in sc.CASES if s in sc.listed(c)}
        assert got == set(sc.FAMILIES), (s, set(sc.FAMILIES) - got)
    for table in (sc.MOVES, sc.SAME_AS_DEFAULT):
        for s, cases in table.items():
            assert s in sc.SETTINGS and set(cases) <= set(sc.CASES), s


@pytest.mark.parametrize('case,setting', sc.pairs(), ids=['%s-%s' % p for p in sc.pairs()])
def test_every_setting_can_be_told_from_the_defaults(case, setting):
    """Its counts differ from the default run's, or its iterate after 40 plain iterations does by more than 1e-4 relative (sigma1e-2 and
    scaling3 leave most counts where the defaults put them)."""
    ok, why = _told_from_the_defaults(case, setting)
    assert ok, (case, setting, why)


def _told_from_the_defaults(case, setting):
    t, t0 = sc.oracle_solve(case, setting)[0], sc.oracle_solve(case, 'default')[0]
    if t != t0:
        return True, (t, t0)
    x, z, y, _ = sc.oracle_iterate(case, setting, 40)
    x0, z0, y0, _ = sc.oracle_iterate(case, 'default', 40)
    d = max(rel(x, x0), rel(z, z0), rel(y, y0))
    return d > 1e-4, (t, d)


def _cases_of(setting):
    return [c for c in sc.CASES if setting in sc.listed(c)]


def test_chk1_ends_off_the_default_round():
    for c in _cases_of('chk1'):
        assert sc.oracle_solve(c, 'chk1')[0][1] % 25 != 0, c


@pytest.mark.parametrize('setting', ['chk10_rho15', 'rho30'])
def test_a_rho_only_stop_refactors_in_every_family(setting):
    """The setting's rho estimates fall between its termination tests (15, 45, ... against 10, 20, ...; 30, 60, ... against 25, 50, ...): every family
    has a case that refactored, and on the headline shape the update came before the first stop the two schedules share (30 / 150), where a
    solve that ends does so before its rho estimate: it was made at a stop that is a rho estimate only."""
    for fam in sc.FAMILIES:
        assert [c for c in _cases_of(setting) if sc.CASES[c]['family'] == fam and sc.oracle_solve(c, setting)[0][2] >= 1], (setting, fam)
    t = sc.oracle_solve('random_12_4_30', setting)[0]
    assert t[2] >= 1 and t[1] <= (30 if setting == 'chk10_rho15' else 150), t


def test_tol15_refactors_more_and_noadapt_never():
    more = [c for c in _cases_of('tol1.5') if sc.oracle_solve(c, 'tol1.5')[0][2] > sc.oracle_solve(c, 'default')[0][2]]
    assert more
    for c in _cases_of('noadapt'):
        assert sc.oracle_solve(c, 'noadapt')[0][2] == 0, c


def test_one_listed_loop_step_runs_into_the_iteration_limit():
    runs = [sc.oracle_loop('random_20_8_12', 'tol1.5', c) for c in range(3)]
    assert any(t[0] == 'maximum iterations reached' and t[1] == 4000 for r in runs for t in r), runs


# ---- the end of a run whose last iteration was not a checked one (osqp_solve: the exact test first, then the 10x one) -----------------------
def test_no_check_until_the_end_still_ends_solved():
    """check_termination = 0, max_iter = 400: 'solved' at 400 wherever the default run is solved by then; a case that needs longer (cart_pole_nc1: 500
    iterations) fails the exact test and gets the 10x test's verdict."""
    for c in _cases_of('chk0'):
        t, t0 = sc.oracle_solve(c, 'chk0')[0], sc.oracle_solve(c, 'default')[0]
        want = 'solved' if t0[1] <= 400 else 'solved inaccurate'
        assert t[:2] == (want, 400), (c, t, t0)
    assert sc.oracle_solve('cart_pole_nc1', 'chk0')[0][0] == 'solved inaccurate'      # (the default run needs 500 iterations)
    assert sc.oracle_solve('random_12_4_30', 'chk0')[0][:2] == ('solved', 400)


def test_a_limit_off_the_round_runs_the_exact_test():
    assert sc.oracle_solve('random_12_4_30', 'max40')[0][:2] == ('solved', 40)
    assert sc.oracle_solve('random_12_4_30', 'default')[0][:2] == ('solved', 50)        # (the checked iterations alone: 25, 50)
    assert sc.oracle_solve('random_5_3_8', 'max60')[0][:2] == ('maximum iterations reached', 60)
    assert sc.oracle_solve('cart_pole', 'max40')[0][:2] == ('solved inaccurate', 40)      # (exact test fails, the 10x one passes)
    assert sc.oracle_solve('random_5_3_8_nc', 'max60')[0][:2] == ('solved', 60)


def test_an_infeasible_problem_at_an_unchecked_limit_is_not_called_inaccurate():
    """The infeasible point mass of tests/test_gpu_parity.py (certificate at iteration 25 with the defaults) stopped at max_iter = 30 with
    check_termination = 0: the exact test finds the certificate."""
    for st in (dict(), dict(check_termination=0, max_iter=30)):
        K = sc.infeasible_point_mass(True, **st)
        assert K.res.info.status == 'primal infeasible' and K.res.info.iter == (30 if st else 25), (st, K.res.info.status, K.res.info.iter)


def test_the_infeasibility_tolerance_moves_the_certificate():
    """What tests/test_gpu_settings.py holds the device to: eps_prim_inf = 1e-7 delays 'primal infeasible' from 25 to 75 iterations; with
    check_termination = 7 from 28 to 119 (four rho updates on the way)."""
    got = [(K.res.info.status, K.res.info.iter) for K in (sc.infeasible_point_mass(True, **st) for st in INFEASIBLE_SETTINGS)]
    assert got == [('primal infeasible', 25), ('primal infeasible', 75), ('primal infeasible', 28), ('primal infeasible', 119)], got


INFEASIBLE_SETTINGS = (dict(), dict(eps_prim_inf=1e-7), dict(check_termination=7), dict(eps_prim_inf=1e-7, check_termination=7))
